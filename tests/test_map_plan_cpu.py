"""Planning through the map without a GPU: the exports and the records' layout; revo_amd.mapfile's restatement
(whole-array min-plus sweeps) against the specification tests/map_plan_ref.py (a heapq Dijkstra) on every shared case, and both
against scipy's Dijkstra on random boxes; the closed form 3a + b + c; what every path must satisfy; the four path statuses;
api.DistanceField.plan / api.CostField on a field without a map, save / load; the `mapfile plan` command on the golden map;
and tests/cpp/plan_host.cpp, the library's host side (argument rules, seed classification, tile geometry, round loop) driven
by a CPU stand-in for the relaxation kernel."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from revo_amd import _lib, api, mapfile
from revo_amd.settings import MapPlanInfo, MapPlanPath, MapPlanSeed, PLAN_NONE

import map_plan_cases as pc
import map_plan_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "small_map.rvm")


def test_declared_exported_and_laid_out(tmp_path):
    for name in ("revo_map_plan", "revo_map_plan_last", "revo_map_plan_paths"):
        assert name in _lib.declared_symbols() and hasattr(_lib.lib(), name)
    recs = {"revo_map_plan_seed": (MapPlanSeed, 16), "revo_map_plan_info": (MapPlanInfo, 64), "revo_map_plan_path": (MapPlanPath, 16)}
    body = ""
    for cname, (cls, _) in recs.items():
        body += '  printf("%s %%zu\\n", sizeof(%s));\n' % (cname, cname)
        for f, _t in cls._fields_:
            body += '  printf("%s.%s %%zu\\n", offsetof(%s, %s));\n' % (cname, f, cname, f)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "revo_hip.h"\nint main(void) {\n%s'
                   '  printf("none %%u\\n", REVO_PLAN_NONE);\n  printf("status %%d %%d %%d %%d\\n", REVO_PLAN_REACHED, REVO_PLAN_UNREACHABLE, '
                   'REVO_PLAN_OUTSIDE, REVO_PLAN_TRUNCATED);\n  return 0;\n}\n' % body)
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    got = dict(ln.split(None, 1) for ln in subprocess.run([str(exe)], capture_output=True, check=True).stdout.decode().splitlines())
    for cname, (cls, size) in recs.items():
        assert int(got[cname]) == size == C.sizeof(cls)
        for f, _t in cls._fields_:
            assert int(got["%s.%s" % (cname, f)]) == getattr(cls, f).offset, (cname, f)
    assert int(got["none"]) == PLAN_NONE == int(mapfile.PLAN_NONE) == pr.NONE
    assert got["status"].split() == ["0", "1", "2", "3"]
    assert (mapfile.PLAN_REACHED, mapfile.PLAN_UNREACHABLE, mapfile.PLAN_OUTSIDE, mapfile.PLAN_TRUNCATED) == (0, 1, 2, 3) == (pr.REACHED, pr.UNREACHABLE, pr.OUTSIDE, pr.TRUNCATED)
    assert [m[:3] for m in pr.MOVES] == list(mapfile.PLAN_MOVES) and mapfile.PLAN_INFO_KEYS == pr.INFO_KEYS


@pytest.mark.parametrize("case", pc.cached_cases(), ids=lambda c: c["name"])
def test_mapfile_follows_the_specification(case):
    want = pr.plan(case["d2"], case["lo"], case["seeds"], case["r2"])
    got = mapfile.plan_records(case["d2"], case["lo"], case["n"], case["seeds"], case["r2"])
    print(case["name"], want[1])
    assert got[0].dtype == np.uint32 and got[0].tobytes() == want[0].tobytes() and got[1] == want[1]
    i = want[1]
    assert i["seeds_used"] + i["seeds_outside"] + i["seeds_blocked"] == len(case["seeds"]) and i["reachable"] <= i["free"] <= i["cells"]
    assert np.all(want[0][case["d2"] < case["r2"]] == pr.NONE)
    assert i["max_cost"] < 2 ** 24 + 5 * 2 ** 27


def test_named_cases_have_their_point():
    by = {c["name"]: c for c in pc.cached_cases()}
    spec = {k: pr.plan(c["d2"], c["lo"], c["seeds"], c["r2"]) for k, c in by.items() if not k.startswith(("a line", "the 40"))}
    assert spec["1 x 1 x 1, free"][0].tolist() == [[[9]]] and spec["1 x 1 x 1, blocked"][1]["seeds_blocked"] == 1
    assert spec["1 x 1 x 1, blocked"][0].tolist() == [[[pr.NONE]]]
    cost, info = spec["a wall across a tile boundary with a one-cell door"]
    assert info["reachable"] == info["free"] and cost[9, 5, 4] == cost[6, 5, 4] + 9  # through the door, straight
    cost, info = spec["two free regions that touch at a tile corner"]
    assert info["reachable"] == info["free"] == 1024 and cost[8, 8, 8] == cost[7, 7, 7] + 5
    cost, info = spec["two free regions that touch at one cell of a tile edge"]
    assert info["reachable"] == info["free"] and cost[8, 8, 0] == cost[7, 7, 0] + 4
    cost, info = spec["an enclosed pocket"]
    assert info["free"] - info["reachable"] == 125 and np.all(cost[4:9, 4:9, 4:9] == pr.NONE)
    cost, info = spec["d2 = r2 and r2 - 1 side by side"]
    assert info["free"] == 6 * 90 + 5 and info["reachable"] == info["free"] and np.all(cost[1::2][:, :4] == pr.NONE)
    info = spec["the seed rules"][1]
    assert (info["seeds_outside"], info["seeds_blocked"], info["seeds_used"]) == (3, 1, 7)
    c = by["the seed rules"]
    cost = spec["the seed rules"][0]
    rel = [tuple(int(a) - int(b) for a, b in zip(s[:3], c["lo"])) for s in c["seeds"]]
    assert cost[rel[4]] == 12 and rel[4] == rel[5] and cost[rel[9]] == 50 and cost[rel[10]] == 53  # the duplicate, the dominated seed
    assert len({tuple(v // 8 for v in r) for r in rel[4:]}) >= 3  # seeds in several tiles
    assert spec["no seed is used"][1]["reachable"] == 0 and spec["no seed is used"][1]["max_cost"] == 0


def test_long_runs():
    line = [c for c in pc.cached_cases() if c["name"].startswith("a line")][0]
    cost, info = mapfile.plan_records(line["d2"], line["lo"], line["n"], line["seeds"], 1)
    assert cost[:, 0, 0].tolist() == [3 * i for i in range(1024)] and info["max_cost"] == 3 * 1023
    s = pc.serpentine()
    want = pr.plan(s["d2"], s["lo"], s["seeds"], 1)
    model, rounds = pr.tile_rounds(s["d2"], s["lo"], s["seeds"], 1)
    print("the serpentine: cost %d at its far end, %d tile rounds in the CPU model" % (want[0][pc.SERPENTINE_FAR], rounds))
    assert model.tobytes() == want[0].tobytes() and want[1]["reachable"] == want[1]["free"]
    # ten corridors of 38 or more cells each: far more than a straight run, and more rounds than the tiles along any way
    assert want[0][pc.SERPENTINE_FAR] == 1162 and rounds == 46 and want[0][pc.SERPENTINE_FAR] > 3 * 10 * 36


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_against_scipy(seed):
    """Random 33 x 20 x 11 boxes at 35 % blocked: the specification, the restatement and scipy's Dijkstra agree."""
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import dijkstra
    c = pc.random_case(seed)
    n = c["n"]
    free = c["d2"] >= 1
    idx = np.arange(free.size).reshape(n)
    rows, cols, w = [], [], []
    for dx, dy, dz, wt in pr.MOVES:
        a = tuple(slice(max(0, -d), n[k] - max(0, d)) for k, d in enumerate((dx, dy, dz)))
        b = tuple(slice(max(0, d), n[k] - max(0, -d)) for k, d in enumerate((dx, dy, dz)))
        ok = free[a] & free[b]
        rows.append(idx[a][ok])
        cols.append(idx[b][ok])
        w.append(np.full(int(ok.sum()), wt, np.float64))
    g = sp.csr_matrix((np.concatenate(w), (np.concatenate(rows), np.concatenate(cols))), shape=(free.size, free.size))
    rel = [tuple(int(a) - int(b) for a, b in zip(s[:3], c["lo"])) for s in c["seeds"]]
    d = dijkstra(g, directed=True, indices=[int(idx[r]) for r in rel], min_only=True).reshape(n)
    want = np.where(np.isfinite(d) & free, d, float(pr.NONE)).astype(np.uint32)
    spec = pr.plan(c["d2"], c["lo"], c["seeds"], 1)
    got = mapfile.plan_records(c["d2"], c["lo"], n, c["seeds"], 1)
    print("seed %d: %d reachable cells" % (seed, spec[1]["reachable"]))
    assert spec[1]["reachable"] > 3000
    assert want.tobytes() == spec[0].tobytes() == got[0].tobytes()


def test_closed_form_in_an_open_box():
    n, s = (9, 7, 6), (2, 5, 1)
    cost, info = mapfile.plan_records(pc.open_box(n), (0, 0, 0), n, [s], 1)
    for c in np.ndindex(*n):
        a, b, d = sorted((abs(c[k] - s[k]) for k in range(3)), reverse=True)
        assert cost[c] == 3 * a + b + d, c
    assert info["reachable"] == info["free"] == info["cells"] == 9 * 7 * 6


def check_paths(case, cost, paths, starts, max_len):
    """What every path must satisfy, from the contract alone."""
    lo, n = np.asarray(case["lo"]), np.asarray(case["n"])
    seeds = {}
    for s in case["seeds"]:
        seeds[s[:3]] = min(seeds.get(s[:3], 1 << 62), s[3])
    seen = set()
    for (cells, status, c0), st in zip(paths, starts):
        seen.add(status)
        rel = np.asarray(st) - lo
        inside = bool(np.all((rel >= 0) & (rel < n)))
        cells = [tuple(int(v) for v in p) for p in cells]
        if not inside:
            assert (status, len(cells), c0) == (pr.OUTSIDE, 0, pr.NONE)
            continue
        v0 = int(cost[tuple(rel)])
        assert c0 == v0
        if v0 == pr.NONE:
            assert (status, len(cells)) == (pr.UNREACHABLE, 0)
            continue
        assert status in (pr.REACHED, pr.TRUNCATED) and cells[0] == tuple(int(v) for v in st) and 1 <= len(cells) <= max_len
        vals = [int(cost[tuple(np.asarray(p) - lo)]) for p in cells]
        for p, q, a, b in zip(cells, cells[1:], vals, vals[1:]):
            d = [abs(x - y) for x, y in zip(p, q)]
            assert max(d) == 1 and a - b == 2 + sum(d)  # 26-adjacent, and the cost falls by exactly the move's weight
        assert all(v != pr.NONE and case["d2"][tuple(np.asarray(p) - lo)] >= case["r2"] for p, v in zip(cells, vals))  # every cell is free
        if status == pr.REACHED:
            assert seeds.get(cells[-1]) == vals[-1]  # a used seed's cell whose cost is its cost0
        else:
            assert len(cells) == max_len
    return seen


@pytest.mark.parametrize("name", ["random 33 x 20 x 11, 35 % blocked, seed 1", "the seed rules", "an enclosed pocket", "the 40 x 40 x 8 serpentine"])
def test_paths(name):
    case = [c for c in pc.cached_cases() if c["name"] == name][0]
    cost, _ = mapfile.plan_records(case["d2"], case["lo"], case["n"], case["seeds"], case["r2"])
    starts = pc.starts_for(case, 64 if name.startswith("the 40") else 256)
    for max_len in (4096, 7):
        want = pr.paths(cost, case["lo"], starts, max_len)
        got = mapfile.plan_paths(cost, case["lo"], case["n"], starts, max_len)
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert g[0].dtype == np.int32 and g[0].shape == (len(w[0]), 3) and [tuple(r) for r in g[0].tolist()] == w[0] and g[1:] == w[1:]
        seen = check_paths(case, cost, got, starts, max_len)
        if name.startswith(("random", "the seed", "an enclosed")):
            assert seen == ({0, 1, 2, 3} if max_len == 7 else {0, 1, 2}), (name, max_len, seen)
    # max_len exactly the path's length and one less
    full = pr.paths(cost, case["lo"], starts, 4096)
    j = max(range(len(full)), key=lambda i: len(full[i][0]))
    L = len(full[j][0])
    assert L > 2
    for ml, status in ((L, pr.REACHED), (L - 1, pr.TRUNCATED)):
        for fn in (pr.paths(cost, case["lo"], [starts[j]], ml), mapfile.plan_paths(cost, case["lo"], case["n"], [starts[j]], ml)):
            assert fn[0][1] == status and [tuple(r) for r in np.asarray(fn[0][0]).tolist()] == full[j][0][:ml]


def test_distance_field_plan_and_cost_field(tmp_path):
    """A DistanceField without a map plans through mapfile; CostField's views, paths in metres, save / load."""
    case = [c for c in pc.cached_cases() if c["name"].startswith("a wall across")][0]
    V = 0.25
    f = api.DistanceField(case["d2"], case["lo"], V)
    cf = f.plan(np.asarray(case["seeds"]), r2=1)
    want = pr.plan(case["d2"], case["lo"], case["seeds"], 1)
    assert isinstance(cf, api.CostField) and cf.cost.tobytes() == want[0].tobytes() and cf.info == want[1] and cf.r2 == 1 and cf.voxel == V
    assert cf.lo.tolist() == list(case["lo"]) and cf.n.tolist() == list(case["n"])
    assert np.array_equal(cf.reachable(), want[0] != pr.NONE)
    m = cf.metres()
    assert m.dtype == np.float32 and np.all(np.isinf(m[~cf.reachable()])) and np.array_equal(m[cf.reachable()], want[0][cf.reachable()].astype(np.float32) * np.float32(V) / np.float32(3))
    # goals as cells, cells with cost0, and points in metres (any point of the cell)
    s = np.asarray(case["seeds"])
    assert f.plan(s[:, :3], r2=1).cost.tobytes() == cf.cost.tobytes()
    assert f.plan((s[:, :3] + 0.3) * V, r2=1).cost.tobytes() == cf.cost.tobytes()
    plus = s.copy()
    plus[:, 3] = 17
    assert np.array_equal(f.plan(plus, r2=1).cost[cf.reachable()], cf.cost[cf.reachable()] + 17)
    # the clearance in metres: r2 = max(1, ceil((clearance / voxel)^2))
    assert [mapfile.plan_r2(x, V) for x in (0.0, 0.1, 0.25, 0.26, 0.5, 0.75)] == [1, 1, 1, 2, 4, 9]
    assert f.plan(s, clearance=0.5).r2 == 4
    with pytest.raises(ValueError):
        f.plan(s)
    with pytest.raises(ValueError):
        f.plan(s, clearance=0.5, r2=4)
    with pytest.raises(ValueError, match="clamp"):
        api.DistanceField(np.minimum(case["d2"], 3), case["lo"], V, clamp=3).plan(s, r2=4)
    assert api.DistanceField(np.minimum(case["d2"], 4), case["lo"], V, clamp=4).plan(s, r2=4).info["free"] == want[1]["free"]
    # paths: cells and metres at the cell centres
    starts = [tuple(int(a) + int(b) for a, b in zip((14, 10, 8), case["lo"])), case["seeds"][0][:3], (1000, 0, 0)]
    p = cf.path(starts)
    w = pr.paths(want[0], case["lo"], starts, 4096)
    assert [([tuple(r) for r in a[0].tolist()], a[1], a[2]) for a in p] == w and [a[1] for a in p] == [0, 0, 2] and len(p[1][0]) == 1
    q = cf.path_points(starts)
    assert q[0][0].dtype == np.float32 and np.array_equal(q[0][0], ((p[0][0].astype(np.float64) + 0.5) * V).astype(np.float32)) and q[0][1:] == p[0][1:]
    assert [a[1] for a in cf.path((np.asarray(starts, np.float64) + 0.5) * V, max_len=3)] == [3, 0, 2]
    # save / load: the same bytes, and a loaded field gives the same paths
    path = str(tmp_path / "c.npz")
    cf.save(path)
    g = api.CostField.load(path)
    assert g.cost.tobytes() == cf.cost.tobytes() and g.lo.tolist() == cf.lo.tolist() and (g.voxel, g.r2, g.info) == (V, 1, None)
    assert [a[0].tolist() for a in g.path(starts)] == [a[0].tolist() for a in p]
    np.savez(str(tmp_path / "bad.npz"), cost=cf.cost)
    with pytest.raises(ValueError):
        api.CostField.load(str(tmp_path / "bad.npz"))
    for bad in (dict(seeds=[(0, 0, 0, -1)]), dict(seeds=[(0, 0, 0, (1 << 24) + 1)]), dict(seeds=np.zeros((0, 3), np.int64)), dict(r2=0)):
        with pytest.raises(ValueError):
            mapfile.plan_records(case["d2"], case["lo"], case["n"], bad.get("seeds", case["seeds"]), bad.get("r2", 1))


def test_mapfile_plan_command(tmp_path, capsys):
    """`mapfile plan` on the golden map: a path between two free cells on opposite sides, the cost file, and clear errors."""
    header, rec = mapfile.read(GOLDEN)
    lo, hi, _ = mapfile.bounds_records(rec)
    clearance = 2.5 * header["voxel"]
    r2 = mapfile.plan_r2(clearance, header["voxel"])
    assert r2 == 7
    blo, bn = mapfile.padded_box(lo, hi, 5)  # ceil(sqrt(7)) + 2
    d2, _ = mapfile.distance_field_records(rec, blo, bn)
    free = np.argwhere(d2 >= r2)
    a, b = free[0] + blo, free[-1] + blo
    solid = mapfile.key_axes(rec["key"])[0]
    out, npz = str(tmp_path / "path.txt"), str(tmp_path / "cost.npz")
    goal, start = ["--goal"] + [str(int(x)) for x in a], ["--start"] + [str(int(x)) for x in b]
    assert mapfile.main(["plan", GOLDEN] + goal + start + ["--start"] + [str(int(x)) for x in solid] + ["--clearance", repr(clearance), "-o", out, "--cost", npz]) == 0
    assert "reached, unreachable" in capsys.readouterr().out
    cf = api.CostField.load(npz)
    want = mapfile.plan_records(d2, blo, bn, [tuple(a)], r2)
    assert cf.cost.tobytes() == want[0].tobytes() and cf.r2 == 7 and cf.lo.tolist() == blo.tolist()
    lines = open(out).read().splitlines()
    heads = [ln for ln in lines if ln.startswith("#")]
    assert len(heads) == 2 and "reached" in heads[0] and "unreachable" in heads[1]
    pts = np.array([[float(x) for x in ln.split()] for ln in lines if not ln.startswith("#")], np.float32)
    p = mapfile.plan_paths(want[0], blo, bn, [tuple(b)], 1 << 20)[0]
    assert p[1] == 0 and np.array_equal(pts, mapfile.plan_path_points(p[0], header["voxel"])) and len(pts) > 3
    assert np.all(d2[tuple((p[0] - blo).T)] >= r2)  # the whole path keeps the clearance
    # nothing reachable: the only start is a solid voxel; the only goal is one; usage errors
    assert mapfile.main(["plan", GOLDEN] + goal + ["--start"] + [str(int(x)) for x in solid] + ["--clearance", "0.0", "--pad", "5", "-o", out]) == 1
    assert "no start reaches a goal" in capsys.readouterr().out
    assert mapfile.main(["plan", GOLDEN, "--goal"] + [str(int(x)) for x in solid] + start + ["--clearance", "0.0", "--pad", "5", "-o", out]) == 1
    assert "no goal lies on a free cell" in capsys.readouterr().out
    assert mapfile.main(["plan", GOLDEN] + goal + start + ["-o", out]) == 2 and mapfile.main(["plan", GOLDEN] + goal + ["--clearance", "0.1", "-o", out]) == 2
    capsys.readouterr()


def _host(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path / "plan_host")
    base = [cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "plan_host.cpp"), "-o", exe]
    # a sanitizer build where the toolchain has one (host code only)
    if subprocess.run(base[:1] + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + base[1:], capture_output=True).returncode != 0:
        subprocess.check_call(base)
    return exe


def test_host_side_follows_the_specification(tmp_path):
    """tests/cpp/plan_host.cpp: the argument rules replayed, then revo_plan_host.h's seed classification, tile geometry and
    round loop over a CPU stand-in for the relaxation kernel -- to the specification's costs and counts, and to
    REVO_ERR_CAPACITY at a limit of one round on the serpentine."""
    exe = _host(tmp_path)
    assert subprocess.run([exe, "rules"], capture_output=True, timeout=120).returncode == 0
    for name, limit in (("the seed rules", 0), ("17 x 17 x 17, 20 % blocked, a seed at every corner", 0), ("d2 = r2 and r2 - 1 side by side", 0),
                        ("the 40 x 40 x 8 serpentine", 0), ("the 40 x 40 x 8 serpentine", 1)):
        c = [x for x in pc.cached_cases() if x["name"] == name][0]
        inp, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(inp, "wb") as f:
            f.write(struct.pack("<6iIII", *c["lo"], *c["n"], c["r2"], len(c["seeds"]), limit))
            f.write(np.asarray(c["seeds"], np.int64).astype(np.int32).tobytes() + c["d2"].tobytes())
        r = subprocess.run([exe, "plan", inp, out], capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        raw = open(out, "rb").read()
        rc, rounds = struct.unpack_from("<iI", raw, 0)
        print("%s at a limit of %d: rc %d after %d rounds" % (name, limit, rc, rounds))
        if limit == 1:
            assert (rc, rounds) == (-5, 1)  # REVO_ERR_CAPACITY
            continue
        want = pr.plan(c["d2"], c["lo"], c["seeds"], c["r2"])
        info = np.frombuffer(raw, np.uint64, 8, 8)
        assert rc == 0 and dict(zip(pr.INFO_KEYS, (int(x) for x in info[:7]))) == want[1] and info[7] == 0
        assert raw[72:] == want[0].tobytes()
        if name.startswith("the 40"):
            assert rounds >= pr.tile_rounds(c["d2"], c["lo"], c["seeds"], 1)[1]  # the loop counts whole groups of rounds
