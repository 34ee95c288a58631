"""The distance field without a GPU: revo_amd.mapfile's separable restatement against the brute-force definition on
every hand-made case and against scipy's exact EDT, df_sample against hand-computed values, bounds_records, the `esdf` command
through api.DistanceField.load, and the ctypes mirrors against the C header."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from revo_amd import api, mapfile
from revo_amd.settings import DF_NONE, MapDfBox, MapDfInfo, MapDfSample

import map_field_cases as fc
import map_field_ref as fr

F = np.float32
RAW = mapfile.RAW_DTYPE
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = F(np.inf)


@pytest.mark.parametrize("case", fc.cases(), ids=lambda c: c["name"])
def test_restatement_equals_the_definition(case):
    rec = fc.records(case["cells"]).astype(RAW)
    got, info = mapfile.distance_field_records(rec, case["lo"], case["n"], case["min_count"], case["clamp"])
    want, winfo = fr.brute_force(rec, case["lo"], case["n"], case["min_count"], case["clamp"])
    assert got.dtype == np.uint32 and got.shape == tuple(case["n"]) and got.tobytes() == want.tobytes()
    assert info == winfo and tuple(info) == mapfile.DF_INFO_KEYS == fr.INFO_KEYS
    if not info["solid"]:
        assert np.all(got == DF_NONE) and info["max_d2"] == 0
    if case["name"].startswith("long axis 0"):
        assert info["max_d2"] == fc.LONG_MAX_FIRST
    if case["name"].startswith("every voxel outside"):
        assert info["outside"] == len(case["cells"])


def test_min_count_excludes_and_counts_below():
    by = {c["min_count"]: c for c in fc.cases() if c["name"].startswith("min_count")}
    rec = fc.records(by[1]["cells"]).astype(RAW)
    f = {mc: mapfile.distance_field_records(rec, c["lo"], c["n"], mc) for mc, c in by.items()}
    assert f[0][0].tobytes() == f[1][0].tobytes() and f[0][1] == f[1][1]
    assert [f[mc][1]["below"] for mc in (1, 2, 3, 4)] == [0, 2, 3, 5]
    assert [f[mc][1]["solid"] for mc in (1, 2, 3, 4)] == [3, 2, 1, 0] and [f[mc][1]["outside"] for mc in (1, 2, 3, 4)] == [2, 1, 1, 0]
    assert f[1][0][1, 1, 1] == 0 and f[2][0][1, 1, 1] == 25 + 1 + 4 and f[3][0][1, 1, 1] == 4 + 16 + 36  # an excluded voxel shortens nothing
    assert np.all(f[4][0] == DF_NONE)


def test_clamp():
    by = {c["clamp"]: c for c in fc.cases() if c["name"].startswith("clamp")}
    rec = fc.records(by[0]["cells"]).astype(RAW)
    free, info = mapfile.distance_field_records(rec, by[0]["lo"], by[0]["n"])
    assert info["max_d2"] < 1000
    for clamp, c in by.items():
        got, i = mapfile.distance_field_records(rec, c["lo"], c["n"], clamp=clamp)
        assert np.array_equal(got, np.minimum(free, clamp) if clamp else free) and i["max_d2"] == (min(info["max_d2"], clamp) if clamp else info["max_d2"])


@pytest.mark.parametrize("shape, voxels", [((70, 45, 37), 300), ((96, 96, 96), 1500)])
def test_restatement_equals_scipy(shape, voxels):
    ndi = pytest.importorskip("scipy.ndimage")
    c = fc.random_case(seed=shape[0], n=shape, voxels=voxels)
    rec = fc.records(c["cells"]).astype(RAW)
    got, info = mapfile.distance_field_records(rec, c["lo"], c["n"])
    occ = np.zeros(shape, bool)
    rel = fr.key_axes(rec["key"]) - np.asarray(c["lo"])
    occ[rel[:, 0], rel[:, 1], rel[:, 2]] = True
    want = np.rint(ndi.distance_transform_edt(~occ) ** 2).astype(np.uint32)
    assert info["solid"] == voxels and np.array_equal(got, want) and info["max_d2"] == int(want.max())


ROOTS = np.array([[0, 1, 4, 9], [2, 3, 8, 10], [7, 5, 6, 20]], np.uint32)  # sqrt of the hand-made field [3, 1, 4] at lo (-1, 2, 0)
LO = (-1, 2, 0)
VOX = 0.5


def _centre(a):
    return [(LO[i] + a[i] + 0.5) * VOX for i in range(3)]


def test_df_sample_by_hand():
    d2 = (ROOTS * ROOTS).reshape(3, 1, 4)
    pts = [_centre(a) for a in ((1, 0, 1), (0, 0, 1), (2, 0, 2), (1, 0, 0), (1, 0, 3))]
    want = [(1.5, (2.0, 0, 3.0)), (0.5, (2.0, 0, 2.0)), (3.0, (-2.0, 0, 7.5)), (1.0, (3.5, 0, 1.0)), (5.0, (5.5, 0, 2.0))]
    got = mapfile.df_sample(d2, LO, VOX, pts)
    assert got.dtype == mapfile.DF_SAMPLE_DTYPE and got.itemsize == 16
    for g, (dist, grad) in zip(got, want):
        assert g["dist"] == F(dist) and g["grad"].tolist() == [F(x) for x in grad]
    # anywhere in the cell, its lower faces included; the upper face belongs to the next cell
    lo_corner = [(LO[i] + 1) * VOX for i in range(3)]
    lo_corner[1] = (LO[1]) * VOX
    assert mapfile.df_sample(d2, LO, VOX, [lo_corner])[0] == got[0]
    # the y faces: an axis of two cells is one-sided on both
    dy = np.array([9, 25], np.uint32).reshape(1, 2, 1)
    g = mapfile.df_sample(dy, (0, 0, 0), VOX, [[0.25, 0.25, 0.25], [0.25, 0.75, 0.25]])
    assert g["dist"].tolist() == [1.5, 2.5] and g["grad"].tolist() == [[0, 2.0, 0], [0, 2.0, 0]]
    # NONE: the cell itself, and as a neighbour (it enters the difference as the number it is)
    dn = d2.copy()
    dn[2, 0, 1] = DF_NONE
    g = mapfile.df_sample(dn, LO, VOX, [_centre((2, 0, 1)), _centre((1, 0, 1))])
    assert g["dist"][0] == INF and not g["grad"][0].any()
    assert g["dist"][1] == F(1.5) and g["grad"][1].tolist() == [F((65536.0 - 1.0) / 2), 0, F(3.0)]
    # outside, on either side of every axis, and not finite
    out = [[-0.5 - 1e-3, 1.25, 0.75], [1.0, 1.25, 0.75], [0.25, 0.999, 0.75], [0.25, 1.5, 0.75], [0.25, 1.25, -1e-6], [0.25, 1.25, 2.0],
           [np.nan, 1.25, 0.75], [0.25, np.inf, 0.75], [0.25, 1.25, -np.inf], [3e38, 1.25, 0.75]]
    g = mapfile.df_sample(d2, LO, VOX, out)
    assert np.all(g["dist"] == F(-1)) and not g["grad"].any()
    assert mapfile.df_sample(d2, LO, VOX, [[-0.5, 1.25, 0.75]])["dist"][0] == F(0.5)  # the lower face of cell (0, 0, 1) is inside
    assert len(mapfile.df_sample(d2, LO, VOX, np.zeros((0, 3)))) == 0


def test_bounds_records():
    rec = fc.records([(1, 1, 1, 1), (-6, 2, 3, 2), (3, 5, -7, 3), (20, 0, 0, 3), (21, -9, 0, 1)]).astype(RAW)
    for mc, lo, hi, n in ((0, (-6, -9, -7), (21, 5, 3), 5), (1, (-6, -9, -7), (21, 5, 3), 5), (2, (-6, 0, -7), (20, 5, 3), 3),
                          (3, (3, 0, -7), (20, 5, 0), 2), (4, (0, 0, 0), (0, 0, 0), 0)):
        b = mapfile.bounds_records(rec, mc)
        assert (b[0].tolist(), b[1].tolist(), b[2]) == (list(lo), list(hi), n) and b[0].dtype == np.int32
    assert mapfile.bounds_records(np.zeros(0, RAW))[2] == 0
    rim = fc.records([(fc.LO_RIM, 0, fc.HI_RIM)]).astype(RAW)
    assert mapfile.bounds_records(rim)[0].tolist() == [fc.LO_RIM, 0, fc.HI_RIM]
    lo, n = mapfile.padded_box(*mapfile.bounds_records(rim)[:2], 8)  # the padding stops at the index range
    assert lo.tolist() == [fc.LO_RIM, -8, fc.HI_RIM - 8] and n.tolist() == [9, 17, 9]


def test_box_limits():
    for lo, n in (((0, 0, 0), (0, 1, 1)), ((0, 0, 0), (1, 1025, 1)), ((0, 0, 0), (1024, 1024, 129)), ((fc.LO_RIM - 1, 0, 0), (2, 2, 2)),
                  ((0, fc.HI_RIM, 0), (2, 2, 2))):
        with pytest.raises(ValueError):
            mapfile.distance_field_records(np.zeros(0, RAW), lo, n)
    assert mapfile.check_box((0, 0, 0), (1024, 1024, 128))[1].tolist() == [1024, 1024, 128]


def test_esdf_command_and_distance_field_files(tmp_path, capsys):
    c = fc.random_case(seed=11, n=(20, 12, 9), voxels=40, counts=True)
    rec = fc.records(c["cells"]).astype(RAW)
    rvm = str(tmp_path / "a.rvm")
    mapfile.write(rvm, mapfile.make_header(fc.V, 0, rec), rec)
    out = str(tmp_path / "f.npz")
    assert mapfile.main(["esdf", rvm, "-o", out, "--pad", "3", "--min-count", "2", "--clamp", "30"]) == 0
    f = api.DistanceField.load(out)
    lo, hi, n = mapfile.bounds_records(rec, 2)
    assert 0 < n < len(rec)
    want, info = mapfile.distance_field_records(rec, lo - 3, hi - lo + 7, 2, 30)
    assert f.d2.tobytes() == want.tobytes() and f.d2.shape == want.shape and f.lo.tolist() == (lo - 3).tolist() and f.n.tolist() == list(want.shape)
    assert f.voxel == fc.V and f.info is None and info["max_d2"] == 30
    with np.load(out) as z:
        assert sorted(z.files) == ["d2", "lo", "n", "voxel"] and z["d2"].dtype == np.uint32 and z["lo"].dtype == z["n"].dtype == np.int32
        assert z["voxel"].dtype == np.float32
    # save / load, metres and sample of a loaded field
    again = str(tmp_path / "g.npz")
    f.save(again)
    g = api.DistanceField.load(again)
    assert g.d2.tobytes() == f.d2.tobytes() and g.lo.tolist() == f.lo.tolist() and g.voxel == f.voxel
    m = f.metres()
    assert m.dtype == F and np.array_equal(m, np.sqrt(want.astype(F)) * F(fc.V))
    pts = (np.asarray(c["cells"])[:5, :3] + 0.5) * fc.V
    assert g.sample(pts).tobytes() == mapfile.df_sample(want, f.lo, fc.V, pts).tobytes()
    assert api.DistanceField(np.full((2, 2, 2), DF_NONE, np.uint32), (0, 0, 0), 1.0).metres().tolist() == [[[np.inf] * 2] * 2] * 2
    # the default pad is 8 cells; a box past the limits is a clear error
    assert mapfile.main(["esdf", rvm, "-o", out]) == 0
    assert api.DistanceField.load(out).n.tolist() == (mapfile.bounds_records(rec)[1] - mapfile.bounds_records(rec)[0] + 17).tolist()
    wide = fc.records([(0, 0, 0), (1100, 0, 0)]).astype(RAW)
    mapfile.write(rvm, mapfile.make_header(fc.V, 0, wide), wide)
    capsys.readouterr()
    assert mapfile.main(["esdf", rvm, "-o", out]) == 1
    assert "1 .. 1024 cells" in capsys.readouterr().out
    assert mapfile.main(["esdf", rvm]) == 2


def test_struct_mirrors_match_the_header(tmp_path):
    assert (C.sizeof(MapDfBox), C.sizeof(MapDfInfo), C.sizeof(MapDfSample)) == (24, 64, 16) and DF_NONE == 0xFFFFFFFF == int(mapfile.DF_NONE)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "revo_hip.h"\n'
                   '#define F(t, m) printf(#t "." #m " %zu\\n", offsetof(t, m));\n'
                   'int main(void) {\n  printf("sizes %zu %zu %zu %u\\n", sizeof(revo_map_df_box), sizeof(revo_map_df_info), sizeof(revo_map_df_sample_t), REVO_DF_NONE);\n'
                   '  F(revo_map_df_box, lo) F(revo_map_df_box, n) F(revo_map_df_info, cells) F(revo_map_df_info, solid) F(revo_map_df_info, outside)\n'
                   '  F(revo_map_df_info, below) F(revo_map_df_info, max_d2) F(revo_map_df_info, reserved) F(revo_map_df_sample_t, dist) F(revo_map_df_sample_t, grad)\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    got = dict(ln.rsplit(" ", 1) if not ln.startswith("sizes") else ("sizes", ln[6:]) for ln in
               subprocess.run([str(exe)], capture_output=True, check=True).stdout.decode().splitlines())
    assert got["sizes"] == "24 64 16 4294967295"
    for t, cls in (("revo_map_df_box", MapDfBox), ("revo_map_df_info", MapDfInfo), ("revo_map_df_sample_t", MapDfSample)):
        for name, _ in cls._fields_:
            assert int(got["%s.%s" % (t, name)]) == getattr(cls, name).offset, (t, name)
    assert [n for n, _ in MapDfInfo._fields_][:5] == list(mapfile.DF_INFO_KEYS)
    from revo_amd import _lib
    for name in ("revo_map_distance_field", "revo_map_bounds", "revo_map_df_sample", "revo_map_distance_field_last_ms"):
        assert name in _lib.declared_symbols()
