"""Views of the TSDF surface without a GPU: the export and the two records' layout; revo_amd.mapfile's vectorised
tsdf_raycast_records against the per-pixel, per-sample loop tests/map_tsdf_ray_ref.py on every shared case, bit for bit; what the
case table covers; the wall's depth bound, the sphere's normals, the colours of a fused volume; views that do not depend on each
other; the refused arguments; the `surface-views` command; and tests/cpp/tsdf_ray_host.cpp, the header host and device code share,
with the march through the block mask against the plain one."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from revo_amd import _lib, api, mapfile, tum
from revo_amd.settings import MapTsdfRayInfo, MapTsdfRayParams

import map_tsdf_cases as tc
import map_tsdf_ray_cases as rc
import map_tsdf_ray_ref as rr

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "small_map.rvm")
IMAGES = ("depth", "normals", "bgr", "status", "samples", "colored")


def same_images(got, want, keys=IMAGES):
    for key in keys:
        assert len(got[key]) == len(want[key]), key
        for i, (g, w) in enumerate(zip(got[key], want[key])):
            assert (g is None) == (w is None), (key, i)
            if g is not None:
                assert g.shape == w.shape and g.dtype == w.dtype and g.tobytes() == w.tobytes(), (key, i)


def test_declared_exported_and_laid_out(tmp_path):
    assert "revo_map_tsdf_raycast" in _lib.declared_symbols() and hasattr(_lib.lib(), "revo_map_tsdf_raycast")
    recs = {"revo_map_tsdf_ray_params": (MapTsdfRayParams, 16), "revo_map_tsdf_ray_info": (MapTsdfRayInfo, 64)}
    body = ""
    for cname, (cls, _) in recs.items():
        body += '  printf("%s %%zu\\n", sizeof(%s));\n' % (cname, cname)
        for f, _t in cls._fields_:
            body += '  printf("%s.%s %%zu\\n", offsetof(%s, %s));\n' % (cname, f, cname, f)
    for i, name in enumerate(("HIT", "RANGE", "BACKFACE", "EXHAUSTED")):
        body += '  printf("status.%s %%u\\n", REVO_TSDF_RAY_%s);\n' % (name, name)
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
    assert [int(got["status.%s" % s.upper()]) for s in rr.STATUS] == [0, 1, 2, 3]
    assert mapfile.TSDF_RAY_STATUS == rr.STATUS and mapfile.TSDF_RAY_INFO_KEYS == rr.INFO_KEYS
    assert [f for f, _ in MapTsdfRayInfo._fields_][:7] == list(rr.INFO_KEYS)


# ------------------------------------------------------------------------------------------------------------- the contract --
@pytest.mark.parametrize("name", list(rc.cases()))
def test_tsdf_raycast_records_follow_the_specification(name):
    c = rc.cases()[name]
    want = rc.spec(name)
    a, kw = rc.args(c)
    got = mapfile.tsdf_raycast_records(*a, **kw)
    print(name, want["info"])
    same_images(got, want)
    assert got["hits"] == want["hits"] and got["info"] == want["info"]
    i = want["info"]
    assert i["rays"] == i["hits"] + i["range"] + i["backface"] + i["exhausted"] == sum(w * h for _, _, (w, h) in c["views"])
    assert sum(want["hits"]) == i["hits"]


def test_the_case_table_covers_the_rules():
    """Conditions on the loop's own results: the cases built to hit do, those built to miss do not, every status occurs, k takes 0, 1
    and 2, and the marked cases meet the situation they were built for."""
    total = dict.fromkeys(rr.INFO_KEYS, 0)
    ks = set()
    for name, c in rc.cases().items():
        w = rc.spec(name)
        if c["kind"] == "hit":
            assert w["info"]["hits"] > 0, name
        if c["kind"] == "miss":
            assert w["info"]["hits"] == 0, name
        for k in rr.INFO_KEYS:
            total[k] += w["info"][k]
        if c["color"] is not None:
            for st, col in zip(w["status"], w["colored"]):
                ks |= set(col[st == rr.HIT].tolist())
    assert all(total[k] > 0 for k in ("hits", "range", "backface", "exhausted")), total
    assert ks == {0, 1, 2}
    # F == 0 is outside: a hit that starts at a sample with Fp == 0 lies at that sample's depth; a backface ends on F == 0
    z = rc.spec("zero sums")
    front = z["depth"][0][z["status"][0] == rr.HIT]
    assert len(front) and np.all(front == F(1.0 / 16.0) + F(8) * F(rc.V)) and np.all(z["status"][1][z["status"][1] != rr.RANGE] == rr.BACKFACE)
    assert (z["status"][1] == rr.BACKFACE).sum() > 0
    # the thin layer is stepped over at three cells a sample and met at one
    assert rc.spec("thin layer stepped over")["info"]["range"] == 192 and rc.spec("thin layer met")["info"]["hits"] > 0
    # the unknown cell takes hits away from its neighbourhood only
    full = dict(rc.cases()["unknown cell between"])
    cells = full["cells"].copy()
    cells["weight"][2, 2, 2] = 1
    whole = rr.raycast(cells, None, full["lo"], rc.V, full["views"])
    assert 0 < rc.spec("unknown cell between")["info"]["hits"] < whole["info"]["hits"]
    # max_steps: one short of the hit's sample exhausts every ray, the exact count reaches it
    assert rc.spec("max_steps one short")["info"]["exhausted"] == 192 and rc.spec("max_steps 1")["info"]["samples"] == 192
    reach, free = rc.spec("max_steps reaches the hit"), rc.spec("9x9x17 block border z")
    assert reach["depth"][0].tobytes() == free["depth"][0].tobytes() and int(free["samples"][0][free["status"][0] == rr.HIT].max()) == 11
    # the hits of the block-border cases lie between the samples at 7.3 and 8.3 cells of the long axis: either side of base 8
    for name in ("9x9x17 block border z", "17x9x9 block border x", "9x17x9 block border y"):
        d = rc.spec(name)["depth"][0]
        u = (d[d > 0] / F(rc.V)) - 2.5
        assert len(u) and np.all((u > 7.3) & (u < 8.3)), name
    # the pixel on the principal point casts (0, 0, 1)
    zd = rc.spec("zero direction components")
    assert zd["status"][0][6, 8] == rr.HIT and np.array_equal(zd["normals"][0][6, 8], F([0, 0, -1]))
    # min_weight 0 counts as 1, 3 leaves fewer valid samples
    assert rc.spec("min_weight 0")["depth"][0].tobytes() == rc.spec("min_weight 1")["depth"][0].tobytes()
    assert rc.spec("min_weight 3")["info"]["hits"] < rc.spec("min_weight 1")["info"]["hits"]


def test_the_wall_is_where_it_was_measured():
    """Every hit's depth lies within trunc / 512 of the wall's depth.  The fused field of one fronto-parallel view is linear in camera
    depth, f = 1024 (D - z) / trunc before rounding, and trilinear interpolation reproduces a linear field; a cell's quantum is rounded
    to the nearest integer, so each of the two samples' fields is off by at most half a quantum and the zero of the line through
    them by less than trunc / 1024 in depth.  The float32 steps on the way (the sample's depth and place, the interpolation, a and
    the product with the step) are relative errors of 2^-24 on numbers of the order of the depth, 1.09 m: far below the bound,
    which is doubled for them."""
    w = tc.wall()
    trunc = float(mapfile.tsdf_trunc(tc.V, w["trunc"]))
    got = rc.spec("wall")
    d = got["depth"][0][got["status"][0] == rr.HIT].astype(np.float64)
    err = np.abs(d - float(tc.WALL_DEPTH))
    print("wall: %d hits, largest |depth - %.2f| = %.3g m, bound trunc / 512 = %.3g m" % (len(d), float(tc.WALL_DEPTH), err.max(), trunc / 512))
    assert len(d) == 35 and err.max() <= trunc / 512
    nrm = got["normals"][0][got["status"][0] == rr.HIT]
    assert np.all(nrm[:, 2] < -0.999)  # the wall faces the camera
    # fused with a colour image, every hit has both colour cells coloured, and the image's colour
    assert np.all(got["colored"][0][got["status"][0] == rr.HIT] == 2) and got["info"]["uncolored"] == 0
    assert np.all(got["bgr"][0][got["status"][0] == rr.HIT] == np.array([17, 130, 251], np.uint8))


def test_the_spheres_normals_face_the_camera():
    got = rc.spec("sphere")
    c = rc.cases()["sphere"]
    o, _, d, _ = mapfile.ray_view_rays(mapfile.ray_view(*c["views"][0]))
    hit = (got["status"][0] == rr.HIT).reshape(-1)
    nrm = got["normals"][0].reshape(-1, 3)
    dots = np.einsum("ij,ij->i", nrm[hit].astype(np.float64), d[hit].astype(np.float64))
    assert hit.sum() > 40 and np.all(dots < 0)
    assert np.allclose(np.linalg.norm(nrm[hit].astype(np.float64), axis=1), 1.0, atol=1e-6) and not nrm[~hit].any()
    # the hits lie on the ball: radius 4.2 cells around the box's middle
    p = o[hit].astype(np.float64) + got["depth"][0].reshape(-1)[hit, None].astype(np.float64) * d[hit].astype(np.float64)
    centre = (np.array(c["lo"]) + 6.0) * rc.V
    assert np.all(np.abs(np.linalg.norm(p - centre, axis=1) / rc.V - 4.2) < 0.2)


def test_a_fused_volume_has_no_uncoloured_hit():
    w = tc.wall()
    tilted = np.eye(4, dtype=F)
    tilted[0, 3] = 0.1
    views = w["views"] + [(w["views"][0][0], tilted, w["views"][0][2])]
    rng = np.random.default_rng(28)
    bgr = [rng.integers(0, 256, (12, 16, 3), dtype=np.uint8) for _ in views]
    cells, _, _, col, _ = mapfile.tsdf_records(tc.V, w["lo"], w["n"], views, w["trunc"], bgr=bgr)
    got = mapfile.tsdf_raycast_records(cells, col, w["lo"], tc.V, [(rc.I4, rc.KC, rc.SIZE), (tilted, rc.KC, rc.SIZE)])
    assert got["info"]["hits"] > 40 and got["info"]["uncolored"] == 0
    assert all(np.all(c[s == rr.HIT] >= 1) for c, s in zip(got["colored"], got["status"]))


def test_views_do_not_depend_on_each_other():
    c = rc.cases()["inside and outside the box"]
    a, kw = rc.args(c)
    together = mapfile.tsdf_raycast_records(*a, **kw)
    total = dict.fromkeys(rr.INFO_KEYS, 0)
    for i, vw in enumerate(c["views"]):
        alone = mapfile.tsdf_raycast_records(c["cells"], c["color"], c["lo"], rc.V, [vw], **kw)
        for key in IMAGES:
            assert alone[key][0].tobytes() == together[key][i].tobytes(), (key, i)
        for k in total:
            total[k] += alone["info"][k]
    assert total == together["info"]
    back = mapfile.tsdf_raycast_records(c["cells"], c["color"], c["lo"], rc.V, c["views"][::-1], **kw)
    assert all(back[key][2 - i].tobytes() == together[key][i].tobytes() for key in IMAGES for i in range(3))
    # without the colour volume only the colours go
    plain = mapfile.tsdf_raycast_records(c["cells"], None, c["lo"], rc.V, c["views"], **kw)
    same_images(plain, together, ("depth", "normals", "status", "samples"))
    assert plain["bgr"] == [None] * 3 and plain["info"] == dict(together["info"], uncolored=0)


def test_refused_arguments():
    c = rc.cases()["3x5x7 lo < 0"]
    view = c["views"][0]
    ok = lambda **kw: mapfile.tsdf_raycast_records(c["cells"], c["color"], c["lo"], rc.V, [view], **kw)  # noqa: E731
    assert ok(step=0)["depth"][0].tobytes() == ok()["depth"][0].tobytes() == ok(step=rc.V, max_steps=0)["depth"][0].tobytes()
    for bad in (dict(step=-0.1), dict(step=float("nan")), dict(step=float("inf")), dict(max_steps=(1 << 20) + 1), dict(max_steps=-1),
                dict(min_weight=-1)):
        with pytest.raises(ValueError):
            ok(**bad)
    assert ok(max_steps=1 << 20)["info"] == ok()["info"]
    T, k, size = view
    nanT = T.copy()
    nanT[0, 3] = np.nan
    bad_views = [[], [view] * 65, [(nanT, k, size)], [(T, k, (0, 12))], [(T, k, (16, 2049))], [(T, (0.0,) + k[1:], size)], [(T, k[:4] + (1.0, 1.0), size)],
                 [(T, k[:4] + (-0.1, 1.0), size)], [(T, k[:5] + (float("inf"),), size)]]
    for views in bad_views:
        with pytest.raises(ValueError):
            mapfile.tsdf_raycast_records(c["cells"], c["color"], c["lo"], rc.V, views)
    for cells, color, lo, voxel in ((c["cells"].view(np.int64), None, c["lo"], rc.V), (c["cells"], c["color"][:-1], c["lo"], rc.V),
                                    (c["cells"], c["cells"], c["lo"], rc.V), (c["cells"], None, ((1 << 20) - 2, 0, 0), rc.V),
                                    (c["cells"], None, c["lo"], 0.0), (c["cells"], None, c["lo"], float("nan"))):
        with pytest.raises(ValueError):
            mapfile.tsdf_raycast_records(cells, color, lo, voxel, [view])
    # the volume's own call
    vol = api.TsdfVolume(c["cells"], c["lo"], rc.V, None, color=c["color"])
    with pytest.raises(ValueError):
        vol.raycast(T)  # without a map the camera must be given
    r = vol.raycast(T, camera=k[:4], size=size, zrange=k[4:])
    assert r["depth"].tobytes() == ok()["depth"][0].tobytes() and r["bgr"].tobytes() == ok()["bgr"][0].tobytes() and r["hits"] == ok()["hits"][0]
    r = vol.raycast([T, T], camera=k[:4], size=size, zrange=k[4:], normals=False, colors=False)
    assert len(r["depth"]) == 2 and r["normals"] is None and r["bgr"] is None and r["info"]["rays"] == 384 and r["info"]["uncolored"] == 0
    assert api.TsdfVolume(c["cells"], c["lo"], rc.V, None).raycast(T, camera=k[:4], size=size, zrange=k[4:])["bgr"] is None


# ------------------------------------------------------------------------------------------------------------------ files --
def test_surface_views_command(tmp_path, capsys):
    header, rec = mapfile.read(GOLDEN)
    lo, hi, _ = mapfile.bounds_records(rec)
    blo, n = mapfile.padded_box(lo, hi, 2)
    voxel = header["voxel"]
    T2 = np.eye(4, dtype=F)
    T2[0, 3] = -0.25
    k = (16.0, 16.0, 31.5, 23.5, 0.1, 5.2)
    depth = float((hi[2] + lo[2]) / 2 * voxel)  # a wall through the middle of the map's bounds
    rng = np.random.default_rng(28)
    views = [(np.full((48, 64), depth + 0.01 * i, F), T, k) for i, T in enumerate((np.eye(4, dtype=F), T2))]
    bgr = [rng.integers(0, 256, (48, 64, 3), dtype=np.uint8) for _ in views]
    cells, _, _, col, _ = mapfile.tsdf_records(voxel, blo, n, views, 0.3, bgr=bgr)
    vol, poses, out = (str(tmp_path / x) for x in ("tsdf.npz", "poses.txt", "views"))
    mapfile.write_tsdf(vol, cells, blo, voxel, 0.3, col)
    T3 = np.eye(4, dtype=F)
    T3[:3, 3] = (0.1, -0.05, 0.2)
    with open(poses, "w") as f:
        for T in (np.eye(4, dtype=F), T3):
            f.write(" ".join("%.9g" % x for x in T.reshape(-1)) + "\n")
    cam = ["--camera", "16", "16", "31.5", "23.5", "--size", "64", "48", "--zrange", "0.1", "5.2"]
    assert mapfile.main(["surface-views", vol, "--poses", poses, "-o", out, "--normals", "--min-weight", "1"] + cam) == 0
    assert "2 views" in capsys.readouterr().out
    rows = tum.read_associate(os.path.join(out, "associate.txt"))
    stated = tum.read_poses(os.path.join(out, "poses.txt"))
    assert [r[0] for r in rows] == [0.0, 1.0] == [ts for ts, _ in stated]
    want = mapfile.tsdf_raycast_records(cells, col, blo, voxel, [(T, k, (64, 48)) for _, T in stated])
    assert want["info"]["hits"] > 2000 and want["info"]["uncolored"] == 0
    for i, (ts, rf, _, df) in enumerate(rows):
        got_bgr, got_depth = tum.load_frame(out, rf, df)
        assert got_bgr.tobytes() == want["bgr"][i].tobytes()
        assert np.array_equal(got_depth, np.clip(np.rint(want["depth"][i].astype(np.float64) * 5000.0), 0, 65535).astype(np.uint16))
        assert np.load(os.path.join(out, "normals", "%.6f.npy" % ts)).tobytes() == want["normals"][i].tobytes()
    # without --normals no such folder; a volume without colour gives black images; a step of its own
    plain, out2 = str(tmp_path / "plain.npz"), str(tmp_path / "views2")
    mapfile.write_tsdf(plain, cells, blo, voxel, 0.3)
    assert mapfile.main(["surface-views", plain, "--poses", poses, "-o", out2, "--step", "0.01"] + cam) == 0
    assert not os.path.exists(os.path.join(out2, "normals"))
    fine = mapfile.tsdf_raycast_records(cells, None, blo, voxel, [(T, k, (64, 48)) for _, T in stated], step=0.01)
    rows = tum.read_associate(os.path.join(out2, "associate.txt"))
    got_bgr, got_depth = tum.load_frame(out2, rows[1][1], rows[1][3])
    assert not got_bgr.any() and np.array_equal(got_depth, np.rint(fine["depth"][1].astype(np.float64) * 5000.0).astype(np.uint16))
    assert mapfile.main(["surface-views", vol, "--poses", poses, "-o", out2, "--step", "-1"] + cam) == 1
    assert mapfile.main(["surface-views", vol, "--poses", poses, "-o", out2]) == 2  # no camera
    capsys.readouterr()


def test_run_tum_surface_views_usage_errors(capsys):
    """The option rules of run_tum --surface-views are decided before any file is read or a device is opened."""
    from revo_amd import run_tum
    base = ["settings.yaml", "dataset.yaml"]
    for extra in (["--map", "0.02", "--surface-views", "dir"],                                       # without --surface
                  ["--map", "0.02", "--surface", "s.ply", "--surface-views-every", "2"],             # without --surface-views
                  ["--map", "0.02", "--surface", "s.ply", "--surface-views", "dir", "--surface-views-every", "0"],
                  ["--surface", "s.ply", "--surface-views", "dir"]):                                 # without --map
        assert run_tum.main(base + extra) == 2, extra
    assert "--surface-views" in capsys.readouterr().out


# ------------------------------------------------------------------------------------------------------- the shared header --
def _host(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path / "tsdf_ray_host")
    base = [cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "tsdf_ray_host.cpp"), "-o", exe]
    # a sanitizer build where the toolchain has one (host code only)
    if subprocess.run(base[:1] + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + base[1:], capture_output=True).returncode != 0:
        subprocess.check_call(base)
    return exe


def _bits(x):
    return int(np.frombuffer(F(x).tobytes(), np.uint32)[0])


HOST_CASES = ("2x2x2", "axis of 1: 5x5x1", "9x9x17 block border z", "17x9x9 block border x", "9x17x9 block border y", "big numbers", "zero sums",
              "unknown cell between", "thin layer stepped over", "behind the wall", "inside and outside the box", "max_steps one short",
              "max_steps reaches the hit", "min_weight 3", "far wall 5x5x33", "far wall 33x5x5", "tilted plane 20x20x20", "sphere",
              "sphere without colour")


def test_host_header(tmp_path):
    """revo_tsdf_ray_host.h: the parameter rules and defaults, a sample's depth from the integer, the coordinate and validity rule at
    the box's rims, the nearest corner at r == 0.5, the decisions at F == 0, the interpolation order against the specification's,
    and the march of the shared cases' rays -- plain against the loop, and through a block mask built from its definition against
    the plain one, line for line."""
    exe = _host(tmp_path)
    voxel = F(rc.V)
    nan, inf = float("nan"), float("inf")
    params = [(0, (9.0, 9, 9, 9)), (1, (0.0, 0, 0, 0)), (1, (0.05, 3, 100, 0)), (1, (1e-3, 0, 1 << 20, 0)), (1, (-0.0, 2, 1, 0)), (1, (-0.5, 0, 0, 0)),
              (1, (nan, 0, 0, 0)), (1, (inf, 0, 0, 0)), (1, (0.1, 0, (1 << 20) + 1, 0)), (1, (0.1, 0, 0, 1))]
    want_params = [[_bits(voxel), 1, 4096], [_bits(voxel), 1, 4096], [_bits(F(0.05)), 3, 100], [_bits(F(1e-3)), 1, 1 << 20], [_bits(voxel), 2, 1]] + [None] * 5
    rng = np.random.default_rng(28)
    depths = [(F(0.1), 0, voxel), (F(0.1), 1 << 20, F(0.01)), (F(0), 7, F(0.3))] + [(F(rng.uniform(0, 2)), int(rng.integers(0, 1 << 20)), F(rng.uniform(1e-3, 0.5)))
                                                                                      for _ in range(30)]
    # o, s, d, lo, n: u = (o + s d) / voxel - (lo + 0.5); the rims are u = 0 and u = n - 1
    axes = [(F(0.0625), F(0), F(1), 0, 5), (np.nextafter(F(0.0625), F(0)), F(0), F(1), 0, 5), (F(0.5625), F(0), F(1), 0, 5),
            (np.nextafter(F(0.5625), F(0)), F(0), F(1), 0, 5), (F(-0.3125), F(1), F(0), -3, 2), (F(-0.3125), F(0.125), F(1), -3, 2),
            (F(0.2), F(0), F(1), 0, 1), (F(nan), F(0), F(1), 0, 5), (F(1), F(inf), F(1), 0, 5), (F(3e38), F(10), F(3e38), 0, 5), (F(-1e-10), F(0), F(1), -1, 9)]
    axes += [(F(rng.uniform(-1, 1)), F(rng.uniform(0, 3)), F(rng.uniform(-1, 1)), int(rng.integers(-9, 3)), int(rng.integers(1, 12))) for _ in range(60)]
    nears = [(3, F(0.5)), (3, np.nextafter(F(0.5), F(0))), (0, F(0)), (-2, F(0.75)), (7, F(1))]
    decides = [(F(0), F(-1)), (F(-1), F(0)), (F(0), F(0)), (F(-0.0), F(-1)), (F(-1), F(-0.0)), (F(2), F(1)), (F(-2), F(-1)), (F(1), F(-1)), (F(-1), F(1)),
               (F(nan), F(-1)), (F(1), F(nan))]
    cubes = []
    for _ in range(40):
        w = rng.choice(np.array([0, 1, 1, 2, 3, 1 << 20], np.int64), 8) if rng.integers(3) == 0 else rng.integers(1, 5, 8)
        s = rng.integers(-(1 << 30), 1 << 30, 8) if rng.integers(2) else rng.integers(-50, 50, 8)
        cubes.append((s, w, F(rng.choice([0.0, 0.5, rng.uniform()])), F(rng.choice([0.0, 0.5, rng.uniform()])), F(rng.uniform()), int(rng.integers(0, 3))))
    blob = struct.pack("<fI", voxel, len(params))
    for has, p in params:
        blob += struct.pack("<IfIII", has, *p)
    blob += struct.pack("<I", len(depths)) + b"".join(struct.pack("<fIf", *x) for x in depths)
    blob += struct.pack("<I", len(axes)) + b"".join(struct.pack("<fffii", *x) for x in axes)
    blob += struct.pack("<I", len(nears)) + b"".join(struct.pack("<if", *x) for x in nears)
    blob += struct.pack("<I", len(decides)) + b"".join(struct.pack("<ff", *x) for x in decides)
    blob += struct.pack("<I", len(cubes))
    for s, w, rx, ry, rz, mw in cubes:
        blob += b"".join(struct.pack("<iI", int(a), int(b)) for a, b in zip(s, w)) + struct.pack("<fffI", rx, ry, rz, mw)
    # the march: every ray of the chosen cases
    blob += struct.pack("<I", len(HOST_CASES))
    want_march = []
    for name in HOST_CASES:
        c = rc.cases()[name]
        step, mw, ms = rr.params(voxel, c["step"], c["min_weight"], c["max_steps"])
        blob += struct.pack("<3i3i", *c["lo"], *c["cells"].shape) + np.ascontiguousarray(c["cells"]).tobytes()
        blob += struct.pack("<I", 0 if c["color"] is None else 1) + (b"" if c["color"] is None else np.ascontiguousarray(c["color"]).tobytes())
        rays = []
        for vw in c["views"]:
            view = mapfile.ray_view(*vw)
            o, s0, d, s1 = mapfile.ray_view_rays(view)
            rays.append(np.concatenate([o, d, s0[:, None], s1[:, None]], 1).astype(F))
        rays = np.concatenate(rays)
        blob += struct.pack("<fIII", step, mw, ms, len(rays)) + rays.tobytes()
        w = rc.spec(name)
        for i in range(len(c["views"])):
            bgr = w["bgr"][i] if w["bgr"][i] is not None else np.zeros(w["depth"][i].shape + (3,), np.uint8)
            for st, sm, dp, nr, px, kc in zip(w["status"][i].ravel(), w["samples"][i].ravel(), w["depth"][i].ravel(), w["normals"][i].reshape(-1, 3),
                                              bgr.reshape(-1, 3), w["colored"][i].ravel()):
                want_march.append([int(st), int(sm), _bits(dp), _bits(nr[0]), _bits(nr[1]), _bits(nr[2]), int(px[0]), int(px[1]), int(px[2]), int(kc)])
    (tmp_path / "in.bin").write_bytes(blob)
    r = subprocess.run([exe, str(tmp_path / "in.bin")], capture_output=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr.decode()[-3000:])
    rows = [ln.split() for ln in r.stdout.decode().splitlines()]
    by = lambda key: [[int(x) for x in row[1:]] if row[1:] != ["refused"] else None for row in rows if row[0] == key]  # noqa: E731
    assert by("params") == want_params
    assert by("s") == [[_bits(F(z + F(F(k) * st)))] for z, k, st in depths]
    want = []
    with np.errstate(all="ignore"):
        for o, s, d, lo, n in axes:
            u = F(F(F(o + F(s * d)) / voxel) - F(F(lo) + F(0.5)))
            b = np.floor(u)
            want.append([1, int(b), _bits(F(u - b))] if np.isfinite(u) and 0 <= b <= n - 2 else [0])
    assert by("axis") == want
    # u == 0 and one step below it; u == n - 1 and one step below it; a box of two cells at u == 0 and at u == 1; an axis of 1; not finite
    assert [w[0] for w in want[:10]] == [1, 0, 0, 1, 1, 0, 0, 0, 0, 0] and want[0][1:] == [0, 0] and want[3][1] == 3 and want[4][1:] == [0, 0]
    assert by("near") == [[4], [3], [0], [-1], [8]]
    assert by("decide") == [[0], [2], [-1], [0], [2], [-1], [-1], [0], [2], [-1], [-1]]
    want = []
    with np.errstate(all="ignore"):
        for s, w, rx, ry, rz, mw in cubes:
            if np.any(w < max(mw, 1)):
                want.append([0, 0, 0, 0, 0, 0])
                continue
            f = {(i >> 2, (i >> 1) & 1, i & 1): F(F(s[i]) / F(w[i])) for i in range(8)}
            Fv, g = rr.interpolate(f, rx, ry, rz)
            want.append([1, _bits(Fv), _bits(g[0]), _bits(g[1]), _bits(g[2]), (4 if rx >= 0.5 else 0) + (2 if ry >= 0.5 else 0) + (1 if rz >= 0.5 else 0)])
    assert by("sample") == want and 10 <= sum(w[0] for w in want) < len(want)  # valid cubes and invalid ones
    assert by("march") == want_march
    assert by("masked") == by("march")
    masks = by("mask")
    assert len(masks) == len(HOST_CASES) and masks[HOST_CASES.index("9x9x17 block border z")] == [1, 1, 2, 2]
    assert masks[HOST_CASES.index("axis of 1: 5x5x1")] == [1, 1, 1, 0]
    assert masks[HOST_CASES.index("far wall 5x5x33")] == [1, 1, 4, 1] and masks[HOST_CASES.index("far wall 33x5x5")] == [4, 1, 1, 1]  # three blocks to step over
    tilted = masks[HOST_CASES.index("tilted plane 20x20x20")]
    assert tilted[:3] == [3, 3, 3] and 0 < tilted[3] < 27
