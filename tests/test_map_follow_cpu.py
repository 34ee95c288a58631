"""A box that follows the camera, without a GPU: the three records' layout from a compiled C snippet; revo_amd.mapfile's
vectorised tsdf_shift_records / tsdf_refill_records against the per-cell loops of tests/map_follow_ref.py on every shared case, bit
for bit; the exact properties (a) and (b); every refusal; SurfaceStore against the loop's dict; the following policy at negative
coordinates and at the index rim; a following run in numpy against the sequence rule; the `surface-assemble` command on a store made
from views of tests/golden/small_map.rvm; and tests/cpp/follow_host.cpp, the header host and device code share."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from revo_amd import _lib, mapfile
from revo_amd.settings import MapTsdfRecord, MapTsdfRefillInfo, MapTsdfShiftInfo

import map_follow_cases as fc
import map_follow_ref as fr

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "small_map.rvm")
CELL, COLOR, RECORD = mapfile.TSDF_CELL_DTYPE, mapfile.TSDF_COLOR_DTYPE, mapfile.TSDF_RECORD_DTYPE


def same(a, b):
    return (a is None and b is None) or (a is not None and b is not None and a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes())


def test_declared_exported_and_laid_out(tmp_path):
    names = ("revo_map_tsdf_shift", "revo_map_tsdf_refill")
    assert all(n in _lib.declared_symbols() and hasattr(_lib.lib(), n) for n in names)
    recs = {"revo_map_tsdf_record": (MapTsdfRecord, 32), "revo_map_tsdf_shift_info": (MapTsdfShiftInfo, 64),
            "revo_map_tsdf_refill_info": (MapTsdfRefillInfo, 32)}
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
    # mapfile's and the loop's record dtypes are the C record, field by field
    for dt in (RECORD, fr.RECORD):
        assert dt.itemsize == 32 and [(f, dt.fields[f][1]) for f in dt.names] == [(f, getattr(MapTsdfRecord, f).offset) for f, _ in MapTsdfRecord._fields_]
    assert mapfile.TSDF_SHIFT_INFO_KEYS == fr.SHIFT_KEYS == tuple(f for f, _ in MapTsdfShiftInfo._fields_)[:5]
    assert mapfile.TSDF_REFILL_INFO_KEYS == fr.REFILL_KEYS == tuple(f for f, _ in MapTsdfRefillInfo._fields_)[:3]


# ------------------------------------------------------------------------------------------------------------- the contract --
@pytest.mark.parametrize("name", list(fc.shift_cases()))
def test_shift_records_follow_the_specification(name):
    c = fc.shift_cases()[name]
    want = fc.shift_spec(name)
    got = mapfile.tsdf_shift_records(c["cells"], c["color"], c["lo"], c["delta"])
    print(name, want[3])
    assert same(got[0], want[0]) and same(got[1], want[1]) and same(got[2], want[2]) and got[3] == want[3]
    assert np.all(got[2]["key"][1:] > got[2]["key"][:-1])
    if c["color"] is None:
        assert not any(got[2][k].any() for k in ("sum_b", "sum_g", "sum_r", "color_weight"))
    # the refill of the records into the emptied source box is the loop's, and gives the leaving cells back
    lo = c["lo"]
    zero = (np.zeros_like(c["cells"]), None if c["color"] is None else np.zeros_like(c["color"]))
    a, b = mapfile.tsdf_refill_records(zero[0], zero[1], lo, got[2]), fr.refill(zero[0], zero[1], lo, want[2])
    assert same(a[0], b[0]) and same(a[1], b[1]) and a[2] == b[2] == {"records": len(want[2]), "applied": len(want[2]), "outside": 0}


def test_the_case_table_covers_what_it_says():
    cases = fc.shift_cases()
    infos = {name: fc.shift_spec(name)[3] for name in cases}
    assert any(i["records"] == 0 and i["leaving"] > 0 for i in infos.values()), "an all-EMPTY volume gives no record"
    assert any(i["staying"] == 0 for i in infos.values()) and any(i["leaving"] == 0 for i in infos.values())
    assert {c["cells"].shape[2] for c in cases.values()} >= {1, 3, 4, 5, 7, 33, 75}
    for nz in (1, 3, 4, 5, 33):
        assert {c["delta"][2] for c in cases.values() if c["cells"].shape == (3, 3, nz) and c["delta"][:2] == (0, 0)} >= set(fc.z_deltas(nz))
    assert any(all(x != 0 for x in c["delta"]) and min(c["delta"]) < 0 < max(c["delta"]) for c in cases.values())
    assert any(c["color"] is None for c in cases.values()) and any(c["color"] is not None for c in cases.values())
    # a cell with weight 0 and a sum that is not 0 is not EMPTY: it leaves as a record
    c = cases["3x5x7 by (1, -2, 3)"]
    assert c["cells"][0, 0, 0]["weight"] == 0 and c["cells"][0, 0, 0]["sum"] != 0
    rec = fc.shift_spec("3x5x7 by (1, -2, 3)")[2]
    assert fr.key(*c["lo"]) in rec["key"].tolist()
    # every hand-set volume FITS
    for c in cases.values():
        assert all(fr.fits(fr.cell_words(c["cells"], c["color"], i)) for i in np.ndindex(*c["cells"].shape))
    assert 300 == int(np.prod(fc.BOX_300[1])) and int(np.prod(fc.BOX_BIG[1])) == 266240 > 1024 * 256


def test_the_large_box_leaving_entirely():
    c = fc.big_case()
    out, cout, rec, info = mapfile.tsdf_shift_records(c["cells"], c["color"], c["lo"], c["delta"])
    assert info == {"cells": 266240, "staying": 0, "leaving": 266240, "records": 266240, "dropped": 0}
    assert not out.view(np.uint8).any() and not cout.view(np.uint8).any()
    # the records are the cells in place order: the key order of one box
    assert np.all(rec["key"][1:] > rec["key"][:-1])
    assert rec["sum"].tobytes() == c["cells"]["sum"].tobytes() and rec["color_weight"].tobytes() == c["color"]["weight"].tobytes()
    assert int(rec["key"][0]) == fr.key(*c["lo"]) and int(rec["key"][-1]) == fr.key(*(l + n - 1 for l, n in zip(c["lo"], fc.BOX_BIG[1])))
    back = mapfile.tsdf_refill_records(out, cout, c["lo"], rec)
    assert same(back[0], c["cells"]) and same(back[1], c["color"])


@pytest.mark.parametrize("name", [n for n in fc.shift_cases() if not n.startswith("fused")])
def test_property_a_there_and_back(name):
    """shift(d), shift(-d), refill(the records) restores both volumes."""
    c = fc.shift_cases()[name]
    d = np.asarray(c["delta"])
    out, cout, rec, _ = mapfile.tsdf_shift_records(c["cells"], c["color"], c["lo"], d)
    back, cback, rec2, info2 = mapfile.tsdf_shift_records(out, cout, np.asarray(c["lo"]) + d, -d)
    assert len(rec2) == 0 and info2["records"] == 0, "what entered was empty"
    res = mapfile.tsdf_refill_records(back, cback, c["lo"], rec)
    assert same(res[0], c["cells"]) and same(res[1], c["color"]) and res[2]["outside"] == 0


@pytest.mark.parametrize("seed,box,d1,d2", fc.composition_cases())
def test_property_b_shifts_compose(seed, box, d1, d2):
    lo, n = box
    cells, col = fc.random_volume(seed, n)
    a = mapfile.tsdf_shift_records(cells, col, lo, d1)
    b = mapfile.tsdf_shift_records(a[0], a[1], np.asarray(lo) + d1, d2)
    whole = mapfile.tsdf_shift_records(cells, col, lo, np.asarray(d1) + d2)
    assert same(b[0], whole[0]) and same(b[1], whole[1])
    both = np.concatenate([a[2], b[2]])
    both = both[np.argsort(both["key"], kind="stable")]
    assert same(both, whole[2]) and len(np.unique(both["key"])) == len(both)


def test_every_refusal():
    cells, col = fc.random_volume(3, (3, 5, 7))
    lo = (-1, -2, 5)
    _, _, rec, _ = mapfile.tsdf_shift_records(cells, col, lo, (1, 0, 2))
    zero, czero = np.zeros_like(cells), np.zeros_like(col)
    assert len(rec) >= 3
    for bad, why in ((rec[::-1], "out of order"), (np.concatenate([rec[:2], rec[1:]]), "a duplicate key"),
                     (np.concatenate([rec[1:], rec[:1]]), "the first record last")):
        for fn, a in ((mapfile.tsdf_refill_records, (zero, czero)), (fr.refill, (zero, czero))):
            with pytest.raises(ValueError):
                fn(a[0], a[1], lo, bad)
    top = rec[:1].copy()
    top["key"] |= np.uint64(1 << 63)
    with pytest.raises(ValueError):
        mapfile.tsdf_refill_records(zero, czero, lo, top)
    # colour words without a colour volume, also for a record outside the box
    coloured = rec[rec["color_weight"] > 0][:1]
    assert len(coloured) == 1
    far = coloured.copy()
    far["key"] = fr.key(1000, 1000, 1000)
    for r in (coloured, far):
        for fn in (mapfile.tsdf_refill_records, fr.refill):
            with pytest.raises(ValueError):
                fn(zero, None, lo, r)
    # a cell that would not FIT: each limit met is accepted, one past it refused, in 64 bits (a sum that 32 bits would wrap)
    one = np.zeros(1, RECORD)
    one["key"] = fr.key(*lo)
    full, cfull = zero.copy(), czero.copy()
    full[0, 0, 0] = (1 << 30, 1 << 20)
    cfull[0, 0, 0] = (255 << 20, 255 << 20, 255 << 20, 1 << 20)
    for field, step in (("sum", 1), ("weight", 1), ("sum_b", 1), ("sum_g", 1), ("sum_r", 1), ("color_weight", 1), ("weight", 0xFFF00000), ("sum_b", 0xFFFFFFFF)):
        r = one.copy()
        r[field] = step
        for fn in (mapfile.tsdf_refill_records, fr.refill):
            with pytest.raises(ValueError):
                fn(full, cfull, lo, r)
            with pytest.raises(ValueError):  # the same record from the other side of the limit
                fn(zero, czero, lo, np.concatenate([r, r]))
    neg = one.copy()
    neg["sum"] = -1
    low = zero.copy()
    low[0, 0, 0] = (-(1 << 30), 0)
    with pytest.raises(ValueError):
        mapfile.tsdf_refill_records(low, czero, lo, neg)
    ok = mapfile.tsdf_refill_records(full, cfull, lo, neg)  # back from the limit
    assert ok[0][0, 0, 0]["sum"] == (1 << 30) - 1 and ok[2] == {"records": 1, "applied": 1, "outside": 0}
    # a record outside the box is not checked for FIT, only counted
    r = far.copy()
    r["weight"] = 0xFFFFFFFF
    assert mapfile.tsdf_refill_records(full, cfull, lo, r)[2] == fr.refill(full, cfull, lo, r)[2] == {"records": 1, "applied": 0, "outside": 1}
    assert mapfile.tsdf_refill_records(full, cfull, lo, rec[:0])[2] == {"records": 0, "applied": 0, "outside": 0}
    # the boxes
    for fn in (mapfile.tsdf_shift_records, fr.shift):
        with pytest.raises(ValueError):
            fn(cells, col, ((1 << 20) - 4, 0, 0), (2, 0, 0))   # the destination passes the rim
        with pytest.raises(ValueError):
            fn(cells, col, (-(1 << 20), 0, 0), (-1, 0, 0))
        with pytest.raises(ValueError):
            fn(cells, col, ((1 << 20) - 2, 0, 0), (0, 0, 0))   # the source does
        assert fn(cells, col, ((1 << 20) - 4, 0, 0), (1, 0, 0))[3]["staying"] == 2 * 5 * 7
    with pytest.raises(ValueError):
        mapfile.tsdf_shift_records(cells, col[:2], lo, (0, 0, 0))


# ---------------------------------------------------------------------------------------------------------------- the store --
def test_the_store():
    cells, col = fc.random_volume(8, (3, 5, 7))
    for vol in (cells, col):  # halved, so that a cell added twice still FITS
        for k in vol.dtype.names:
            vol[k] //= 2
    lo = np.array((-1, -2, 5))
    _, _, r1, _ = mapfile.tsdf_shift_records(cells, col, lo, (1, 0, 0))
    _, _, r2, _ = mapfile.tsdf_shift_records(cells, col, lo, (0, 0, 3))   # shares a corner line with r1: equal keys are summed
    assert len(np.intersect1d(r1["key"], r2["key"])) > 0
    s, w = mapfile.SurfaceStore(voxel=fc.V, trunc=0.5), fr.Store()
    assert len(s) == 0 and s.bounds() is None
    for r in (r1, r2, r1[:0]):
        s.add(r)
        w.add(r)
    assert same(s.records, w.records()) and len(s) == len(w.cells) == len(np.union1d(r1["key"], r2["key"]))
    b, wb = s.bounds(), w.bounds()
    assert np.array_equal(b[0], wb[0]) and np.array_equal(b[1], wb[1])
    for box in ((lo, (3, 5, 7)), ((0, 0, 0), (2, 2, 2)), ((-1, -2, 9), (4, 2, 6))):
        got, want = s.volume(*box), w.volume(*box)
        assert same(got[0], want[0]) and same(got[1], want[1])
    # all or nothing: a summed cell that would not FIT leaves the store as it was
    big = s.records[:1].copy()
    big["weight"] = (1 << 20) - int(big["weight"][0]) + 1
    for st in (s, w):
        with pytest.raises(ValueError):
            st.add(np.concatenate([s.records[1:2], big]))
    assert same(s.records, w.records())
    with pytest.raises(ValueError):
        s.volume(lo, (3, 5, 7), voxel=0.25)
    with pytest.raises(ValueError):
        s.volume(lo, (3, 5, 7), trunc=0.25)
    # the npz round trip
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        p = s.save(os.path.join(d, "store.npz"))
        t = mapfile.SurfaceStore.load(p)
        assert same(t.records, s.records) and t.voxel == s.voxel == float(F(fc.V)) and t.trunc == 0.5
        np.savez(os.path.join(d, "bad.npz"), records=s.records[::-1], voxel=F(1), trunc=F(1))
        with pytest.raises(ValueError):
            mapfile.SurfaceStore.load(os.path.join(d, "bad.npz"))
    # take removes what it returns, in key order
    box = ((-1, -2, 5), (1, 5, 7))
    got, want = s.take(*box), w.take(*box)
    assert same(got, want) and len(got) > 0 and same(s.records, w.records()) and len(s.take(*box)) == 0
    assert not np.any(np.isin(got["key"], s.records["key"]))
    # what is taken refills the box it was taken for
    out = mapfile.tsdf_refill_records(np.zeros((1, 5, 7), CELL), np.zeros((1, 5, 7), COLOR), box[0], got)
    assert out[2]["outside"] == 0


def test_follow_lo():
    n = (12, 10, 8)
    at = lambda t, R=np.eye(3): np.vstack([np.hstack([np.asarray(R, F), np.asarray(t, F).reshape(3, 1)]), F([[0, 0, 0, 1]])])  # noqa: E731
    assert mapfile.follow_lo(at((0, 0, 0)), n, fc.V, 0.5, 2).tolist() == [-6, -6, 0] == fr.follow_lo(at((0, 0, 0)), n, fc.V, 0.5, 2)
    # negative coordinates: floor, not truncation, in the cell index and in the snap
    assert mapfile.follow_lo(at((-0.01, -0.13, -0.51)), n, fc.V, 0.5, 2).tolist() == [-8, -8, -6]  # cells -1, -2, -1 -> want -7, -7, -5
    assert mapfile.follow_lo(at((-0.01, -0.13, -0.51)), n, fc.V, 0.5, 1).tolist() == [-7, -7, -5]
    assert mapfile.follow_lo(at((-0.01, -0.13, -0.51)), n, fc.V, 0.5, 16).tolist() == [-16, -16, -16]
    # the camera's z axis, not the world's
    Ry = [[0, 0, 1], [0, 1, 0], [-1, 0, 0]]  # looks down +x
    assert mapfile.follow_lo(at((0, 0, 0), Ry), n, fc.V, 0.5, 2).tolist() == [-2, -6, -4]
    # the rim: clamped so the box stays inside the index range
    far = (1 << 20) * fc.V
    assert mapfile.follow_lo(at((far, -far - 100.0, 0)), n, fc.V, 0.5, 2).tolist() == [(1 << 20) - 12, -(1 << 20), 0]
    rng = np.random.default_rng(5)
    for _ in range(200):
        T = at(rng.uniform(-300, 300, 3), np.linalg.qr(rng.normal(size=(3, 3)))[0])
        step, ahead = int(rng.integers(1, 20)), float(rng.uniform(-1, 3))
        got = mapfile.follow_lo(T, n, fc.V, ahead, step)
        assert got.tolist() == fr.follow_lo(T, n, fc.V, ahead, step)
        mapfile.check_box(got, n)
    with pytest.raises(ValueError):
        mapfile.follow_lo(at((0, 0, 0)), n, fc.V, 0.5, 0)
    with pytest.raises(ValueError):
        mapfile.follow_lo(at((np.nan, 0, 0)), n, fc.V, 0.5, 2)


def follow_in_numpy(views, n, step, ahead, voxel, trunc):
    """A following run through mapfile alone: -> (store, cells, colour, lo, the box each view was fused in, shifts)."""
    store = mapfile.SurfaceStore(voxel=voxel, trunc=trunc)
    shape = tuple(int(x) for x in n)
    cells, col, lo, boxes, shifts = np.zeros(shape, CELL), np.zeros(shape, COLOR), None, [], 0
    for depth, T, k, bgr in views:
        new = mapfile.follow_lo(T, n, voxel, ahead, step)
        if lo is not None and np.any(new != lo):
            cells, col, rec, _ = mapfile.tsdf_shift_records(cells, col, lo, new - lo)
            store.add(rec)
            cells, col, _ = mapfile.tsdf_refill_records(cells, col, new, store.take(new, n))
            shifts += 1
        lo = new
        cells, _, _, col, _ = mapfile.tsdf_records(voxel, lo, n, [(depth, T, k)], trunc, tsdf=cells, bgr=[bgr], color=col)
        boxes.append(lo.copy())
    return store, cells, col, lo, boxes, shifts


def assemble_in_numpy(store, cells, col, lo):
    whole = mapfile.SurfaceStore(store.records, store.voxel, store.trunc)
    whole.add(mapfile.tsdf_volume_records(cells, col, lo))
    return whole


@pytest.fixture(scope="module")
def follow_run():
    views = fc.follow_views()
    return views, follow_in_numpy(views, fc.FOLLOW_N, fc.FOLLOW_STEP, 0.5, fc.V, 0.5)


def test_a_following_run_is_the_sequence_rule(follow_run):
    views, (store, cells, col, lo, boxes, shifts) = follow_run
    print("boxes", [b.tolist() for b in boxes], "shifts", shifts, "store", len(store))
    assert shifts >= 3 and boxes[0].tolist() == boxes[-1].tolist() == lo.tolist()
    assert all(len({b[k] for b in map(tuple, boxes)}) > 1 for k in range(3)), "the box moves on every axis"
    want = fr.sequence(fc.V, fc.FOLLOW_N, [v[:3] for v in views], [v[3] for v in views], boxes, 0.5)
    whole = assemble_in_numpy(store, cells, col, lo)
    blo, bn = whole.bounds()
    got = whole.volume(blo, bn)
    ref = fr.sequence_volume(want, blo, bn)
    assert same(got[0], ref[0]) and same(got[1], ref[1]) and len(whole) == len(want) > 0
    assert len(store) > 0 and not np.any(store._inside(lo, fc.FOLLOW_N)), "what lies in the box is in the box, not in the store"


def test_surface_assemble_command(tmp_path, capsys):
    header, rec = mapfile.read(GOLDEN)
    voxel = header["voxel"]
    mlo, mhi, _ = mapfile.bounds_records(rec)
    mid = (np.asarray(mlo, np.float64) + np.asarray(mhi)) / 2.0 * voxel
    k = (8.5, 8.5, 7.5, 5.5, 0.1, 5.2)
    poses = []
    for dx in (-1.5, 0.0, 1.5, 0.0):  # along the map's long axis and back, from in front of it
        T = np.eye(4, dtype=F)
        T[:3, 3] = F(mid + (dx, 0.0, -2.5))
        poses.append(T)
    cast = mapfile.raycast_records(rec, voxel, [(T, k, (16, 12)) for T in poses])
    assert min(cast["hits"]) > 0
    views = [(d, T, k, im) for d, T, im in zip(cast["depth"], poses, cast["bgr"])]
    n, trunc = (12, 10, 8), 1.0
    store, cells, col, lo, boxes, shifts = follow_in_numpy(views, n, 2, 2.5, voxel, trunc)
    assert shifts == 3 and len(store) > 0
    whole = assemble_in_numpy(store, cells, col, lo)
    want = fr.sequence(voxel, n, [v[:3] for v in views], [v[3] for v in views], boxes, trunc)
    assert len(whole) == len(want) > 0
    p, out = str(tmp_path / "store.npz"), str(tmp_path / "tsdf.npz")
    whole.save(p)
    assert mapfile.main(["surface-assemble", p, "-o", out]) == 0
    assert "cells from" in capsys.readouterr().out
    got, glo, gv, gt, gcol = mapfile.read_tsdf(out, color=True)
    blo, bn = whole.bounds()
    ref = fr.sequence_volume(want, blo, bn)
    assert glo.tolist() == blo.tolist() and gv == voxel and gt == trunc and same(got, ref[0]) and same(gcol, ref[1])
    assert int((got["weight"] > 0).sum()) > 0 and int((gcol["weight"] > 0).sum()) > 0
    assert mapfile.main(["mesh", out, "-o", str(tmp_path / "mesh.ply"), "--normals", "--colors"]) == 0, "the file is what `mapfile mesh` reads"
    # a box of one's own
    box = [int(x) for x in lo] + [12, 10, 8]
    assert mapfile.main(["surface-assemble", p, "--box"] + [str(x) for x in box] + ["-o", out]) == 0
    got, glo, _, _, gcol = mapfile.read_tsdf(out, color=True)
    assert same(got, cells) and same(gcol, col) and glo.tolist() == lo.tolist()
    capsys.readouterr()
    # refused with a message: an axis above 1024 cells, more than 2^27 cells, an empty store, no store at all
    wide = mapfile.SurfaceStore(whole.records[:1], voxel, trunc)
    r = whole.records[-1:].copy()
    r["key"] = fr.key(int(blo[0]) + 1024, int(blo[1]), int(blo[2]))
    wide.add(r)
    wide.save(p)
    assert mapfile.main(["surface-assemble", p, "-o", out]) == 1 and "1024" in capsys.readouterr().out
    assert mapfile.main(["surface-assemble", p, "--box", "0", "0", "0", "1024", "1024", "512", "-o", out]) == 1 and "2^27" in capsys.readouterr().out
    mapfile.SurfaceStore(voxel=voxel, trunc=trunc).save(p)
    assert mapfile.main(["surface-assemble", p, "-o", out]) == 1 and "empty" in capsys.readouterr().out
    assert mapfile.main(["surface-assemble", GOLDEN, "-o", out]) == 1 and mapfile.main(["surface-assemble", p]) == 2
    capsys.readouterr()


# ------------------------------------------------------------------------------------------------------- the shared header --
def test_host_header(tmp_path):
    """revo_tsdf_follow_host.h against brute force: the staying sub-box, the leaving rank and its inverse on small boxes at every shift up
    to one past the box, EMPTY, FITS at its four limits and one past each, the key."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path / "follow_host")
    base = [cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "follow_host.cpp"), "-o", exe]
    # a sanitizer build where the toolchain has one (host code only)
    if subprocess.run(base[:1] + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + base[1:], capture_output=True).returncode != 0:
        subprocess.check_call(base)
    r = subprocess.run([exe], capture_output=True, timeout=120)
    out = r.stdout.decode()
    assert r.returncode == 0 and out.split() == ["shifts", "5275", "empty", "fits", "keys", "ok"], out + r.stderr.decode()[-2000:]
    # the limits the header states are mapfile's and the loop's
    hdr = open(os.path.join(ROOT, "revo_amd", "csrc", "revo_tsdf_follow_host.h")).read()
    assert "#define FOLLOW_W_MAX (1u << 20)" in hdr and "#define FOLLOW_SUM_MAX (1ll << 30)" in hdr and "#define FOLLOW_COLOR_MAX (255ll << 20)" in hdr
    assert (mapfile.TSDF_W_MAX, mapfile.TSDF_SUM_MAX, mapfile.TSDF_COLOR_MAX) == (fr.W_MAX, fr.SUM_MAX, fr.COLOR_MAX) == (1 << 20, 1 << 30, 255 << 20)
