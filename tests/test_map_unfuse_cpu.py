"""Views taken out of the TSDF surface again, without a GPU: the export and the record's layout;
revo_amd.mapfile.tsdf_unfuse_records against the per-cell specification (tests/map_tsdf_ref.py, map_surface_ref.py) on every shared
case -- fuse all, take out the removed, and the bytes are those of fusing the kept -- with and without colour; every refusal with
its exact number of misfits and untouched inputs; the refused arguments; api.TsdfVolume.unfuse without a map; the tsdf-unfuse
command; and tests/cpp/tsdf_unfuse_host.cpp, the per-cell rule host and device code share, built with the host sanitizers."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from revo_amd import _lib, api, mapfile
from revo_amd.settings import MapTsdfUnfuseInfo

import map_surface_ref as sf
import map_tsdf_cases as tc
import map_tsdf_ref as tr
import map_unfuse_cases as uc

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_export_and_the_record(tmp_path):
    assert "revo_map_tsdf_unfuse" in _lib.declared_symbols() and hasattr(_lib.lib(), "revo_map_tsdf_unfuse")
    body = '  printf("size %zu\\n", sizeof(revo_map_tsdf_unfuse_info));\n'
    for f, _t in MapTsdfUnfuseInfo._fields_:
        body += '  printf("%s %%zu\\n", offsetof(revo_map_tsdf_unfuse_info, %s));\n' % (f, f)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "revo_hip.h"\nint main(void) {\n%s  return 0;\n}\n' % body)
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    got = dict(ln.split() for ln in subprocess.run([str(exe)], capture_output=True, check=True).stdout.decode().splitlines())
    assert int(got["size"]) == 64 == C.sizeof(MapTsdfUnfuseInfo)
    for i, (f, _t) in enumerate(MapTsdfUnfuseInfo._fields_):
        assert int(got[f]) == getattr(MapTsdfUnfuseInfo, f).offset == 8 * i
    assert tuple(f for f, _ in MapTsdfUnfuseInfo._fields_)[:7] == mapfile.TSDF_UNFUSE_INFO_KEYS
    L = _lib.lib()
    assert L.revo_map_tsdf_unfuse(None, None, 0, None, None, 0, 0.0, None, None, 0, None, None) == -1  # no device needed


def _zero(a):
    return not np.ascontiguousarray(a).view(np.uint8).any()


@pytest.mark.parametrize("name", list(uc.cases()))
def test_unfuse_records_inverts_the_fuse(name):
    c = uc.cases()[name]
    all_cells, all_col = uc.fused(name, "all")
    want_cells, want_col = uc.fused(name, "kept")
    views, bgr = uc.pick(c, c["removed"])
    for color in (True, False):
        before = (all_cells.copy(), all_col.copy())
        cells, col, info, counts = mapfile.tsdf_unfuse_records(all_cells, all_col if color else None, c["lo"], uc.V, views, c["trunc"],
                                                               bgr=bgr if color else None)
        assert cells.dtype == tr.CELL and cells.tobytes() == want_cells.tobytes(), (name, color, int(np.sum(cells != want_cells)))
        assert (col is None) if not color else (col.dtype == sf.COLOR and col.tobytes() == want_col.tobytes()), (name, color)
        assert all_cells.tobytes() == before[0].tobytes() and all_col.tobytes() == before[1].tobytes()  # the inputs are not changed
        # the counters, from the two volumes; the per-view counts are the fuse's
        assert info == {"cells": cells.size, "updates": int(all_cells["weight"].sum()) - int(want_cells["weight"].sum()),
                        "cells_weighted": int((want_cells["weight"] > 0).sum()), "misfits": 0,
                        "cells_inside": int(((want_cells["weight"] > 0) & (want_cells["sum"] < 0)).sum()),
                        "color_updates": int(all_col["weight"].sum()) - int(want_col["weight"].sum()) if color else 0,
                        "cells_colored": int((want_col["weight"] > 0).sum()) if color else 0}, (name, color, info)
        assert counts == mapfile.tsdf_records(uc.V, c["lo"], c["n"], views, c["trunc"])[2]
        if not c["kept"]:
            assert _zero(cells) and (col is None or _zero(col))
    if name == "9x7x5 trunc M / every second":  # in two steps, either order, and the removed views fused back: the round trip
        half = len(views) // 2
        step = mapfile.tsdf_unfuse_records(all_cells, all_col, c["lo"], uc.V, views[half:], c["trunc"], bgr=bgr[half:])
        step = mapfile.tsdf_unfuse_records(step[0], step[1], c["lo"], uc.V, views[:half], c["trunc"], bgr=bgr[:half])
        assert step[0].tobytes() == want_cells.tobytes() and step[1].tobytes() == want_col.tobytes()
        back = mapfile.tsdf_records(uc.V, c["lo"], c["n"], views, c["trunc"], tsdf=step[0], bgr=bgr, color=step[1])
        assert back[0].tobytes() == all_cells.tobytes() and back[3].tobytes() == all_col.tobytes()


@pytest.mark.parametrize("name", list(uc.refusals()))
def test_refusals_count_the_misfits_and_touch_nothing(name):
    r = uc.refusals()[name]
    tried = 0
    for color in (True, False):
        if (color and r.get("tsdf_only")) or (not color and r.get("color_only")):
            continue
        cells, col = r["cells"].copy(), r["color"].copy()
        with pytest.raises(mapfile.TsdfUnfuseRefused) as e:
            mapfile.tsdf_unfuse_records(cells, col if color else None, r["lo"], uc.V, r["views"], r["trunc"], bgr=r["bgr"] if color else None)
        assert e.value.misfits == r["misfits"] == e.value.info["misfits"], (name, color, e.value.misfits)
        assert e.value.info["updates"] == 0 == e.value.info["color_updates"] and e.value.info["cells"] == cells.size
        assert e.value.info["cells_weighted"] == int((cells["weight"] > 0).sum())
        assert e.value.info["cells_colored"] == (int((col["weight"] > 0).sum()) if color else 0)
        assert cells.tobytes() == r["cells"].tobytes() and col.tobytes() == r["color"].tobytes()
        tried += 1
    assert tried
    if r.get("color_only") and r.get("tsdf_fits", True):  # the TSDF rule alone has nothing against it
        out = mapfile.tsdf_unfuse_records(r["cells"], None, r["lo"], uc.V, r["views"], r["trunc"])
        assert out[2]["misfits"] == 0 and out[1] is None


def test_refused_arguments_and_the_default_trunc():
    c = uc.cases()["3x5x7 default trunc / first"]
    cells, col = uc.fused("3x5x7 default trunc / first", "all")
    views, bgr = uc.pick(c, c["removed"])
    for bad in (lambda: mapfile.tsdf_unfuse_records(cells, col, c["lo"], uc.V, views),                      # colour volume without images
                lambda: mapfile.tsdf_unfuse_records(cells, None, c["lo"], uc.V, views, bgr=bgr),             # images without a colour volume
                lambda: mapfile.tsdf_unfuse_records(cells, col, c["lo"], uc.V, views, bgr=bgr + bgr),       # one image per view
                lambda: mapfile.tsdf_unfuse_records(cells, col[:-1], c["lo"], uc.V, views, bgr=bgr),
                lambda: mapfile.tsdf_unfuse_records(cells, None, c["lo"], uc.V, views, trunc=-1.0),
                lambda: mapfile.tsdf_unfuse_records(cells, None, c["lo"], uc.V, views, trunc=float("nan")),
                lambda: mapfile.tsdf_unfuse_records(cells, None, c["lo"], uc.V, []),
                lambda: mapfile.tsdf_unfuse_records(cells, None, c["lo"], uc.V, views * 65),
                lambda: mapfile.tsdf_unfuse_records(cells["sum"], None, c["lo"], uc.V, views)):
        with pytest.raises(ValueError) as e:
            bad()
        assert not isinstance(e.value, mapfile.TsdfUnfuseRefused)
    # None and 0 both mean 4 x the voxel edge
    a = mapfile.tsdf_unfuse_records(cells, col, c["lo"], uc.V, views, None, bgr=bgr)
    b = mapfile.tsdf_unfuse_records(cells, col, c["lo"], uc.V, views, 0.0, bgr=bgr)
    d = mapfile.tsdf_unfuse_records(cells, col, c["lo"], uc.V, views, 4 * uc.V, bgr=bgr)
    assert a[0].tobytes() == b[0].tobytes() == d[0].tobytes() and a[1].tobytes() == b[1].tobytes() == d[1].tobytes()


def test_volume_without_a_map():
    c = uc.cases()["two views / last"]
    cells, col = uc.fused("two views / last", "all")
    want = uc.fused("two views / last", "kept")
    views, bgr = uc.pick(c, c["removed"])
    vol = api.TsdfVolume(cells, c["lo"], uc.V, c["trunc"], color=col)
    got = vol.unfuse([tuple(v) + (im,) for v, im in zip(views, bgr)])
    assert got.cells.tobytes() == want[0].tobytes() and got.color.tobytes() == want[1].tobytes() and got.info["misfits"] == 0
    assert got.trunc == vol.trunc and np.array_equal(got.lo, vol.lo) and vol.cells.tobytes() == cells.tobytes()
    plain = api.TsdfVolume(cells, c["lo"], uc.V, c["trunc"]).unfuse(views)
    assert plain.color is None and plain.cells.tobytes() == want[0].tobytes()
    with pytest.raises(mapfile.TsdfUnfuseRefused):
        got.unfuse([tuple(v) + (im,) for v, im in zip(views, bgr)])


def test_command_line(tmp_path, capsys):
    from PIL import Image
    from revo_amd import vo
    folder, full, out = (str(tmp_path / x) for x in ("views", "full.npz", "out.npz"))
    os.makedirs(os.path.join(folder, "depth"))
    os.makedirs(os.path.join(folder, "rgb"))
    k = tc.KC
    lo, n, trunc = tc.LO, tc.N, 0.25
    rng = np.random.default_rng(32)
    views, bgr, stamps = [], [], []
    for i in range(3):
        T = np.eye(4, dtype=F)
        T[0, 3] = F(0.0625) * i
        stamps.append((1.5 + i, T))
    with open(os.path.join(folder, "poses.txt"), "w") as f:
        f.write("".join(line + "\n" for line in vo.tum_lines(stamps)))
    with open(os.path.join(folder, "associate.txt"), "w") as f:
        for i, (ts, T) in enumerate(stamps):
            raw = np.rint((1.0 + 0.05 * i + 0.01 * rng.random((12, 16))) * 5000.0).astype(np.uint16)
            im = rng.integers(0, 256, (12, 16, 3), dtype=np.uint8)
            name = "%.6f.png" % ts
            Image.fromarray(raw).save(os.path.join(folder, "depth", name))
            Image.fromarray(np.ascontiguousarray(im[..., ::-1])).save(os.path.join(folder, "rgb", name))  # the file holds R, G, B
            f.write("%.6f rgb/%s %.6f depth/%s\n" % (ts, name, ts, name))
            views.append((raw.astype(F) / F(5000.0), T, k))
            bgr.append(im)
    cam = ["--camera"] + [str(x) for x in k[:4]] + ["--zrange", str(k[4]), str(k[5])]
    whole = mapfile.tsdf_records(uc.V, lo, n, views, trunc, bgr=bgr)
    assert whole[1]["cells_inside"] > 0 and whole[4]["cells_colored"] > 0
    mapfile.write_tsdf(full, whole[0], lo, uc.V, trunc, whole[3])
    assert mapfile.main(["tsdf-unfuse", full, "--views", folder, "--only", "0,2", "-o", out] + cam) == 0
    want = mapfile.tsdf_records(uc.V, lo, n, views[1:2], trunc, bgr=bgr[1:2])
    cells, tlo, voxel, tr_, col = mapfile.read_tsdf(out, color=True)
    assert cells.tobytes() == want[0].tobytes() and col.tobytes() == want[3].tobytes() and (voxel, tr_) == (uc.V, trunc) and list(tlo) == list(lo)
    assert "taken out" in capsys.readouterr().out
    # everything out: zeros; a volume without colour takes the depth images alone
    zero = str(tmp_path / "zero.npz")
    assert mapfile.main(["tsdf-unfuse", full, "--views", folder, "-o", zero] + cam) == 0
    z = mapfile.read_tsdf(zero, color=True)
    assert _zero(z[0]) and _zero(z[4])
    plain, plain_out = str(tmp_path / "plain.npz"), str(tmp_path / "plain_out.npz")
    mapfile.write_tsdf(plain, whole[0], lo, uc.V, trunc)
    assert mapfile.main(["tsdf-unfuse", plain, "--views", folder, "--only", "1", "-o", plain_out] + cam) == 0
    got = mapfile.read_tsdf(plain_out, color=True)
    assert got[4] is None and got[0].tobytes() == mapfile.tsdf_records(uc.V, lo, n, [views[0], views[2]], trunc)[0].tobytes()
    # refused: the views are no longer in it; nothing is written.  Usage errors
    again = str(tmp_path / "again.npz")
    assert mapfile.main(["tsdf-unfuse", out, "--views", folder, "--only", "0", "-o", again] + cam) == 1 and not os.path.exists(again)
    assert "refused" in capsys.readouterr().out
    assert mapfile.main(["tsdf-unfuse", full, "--views", folder, "--only", "7", "-o", again] + cam) == 1
    assert mapfile.main(["tsdf-unfuse", full, "-o", again]) == 2 and mapfile.main(["tsdf-unfuse", full, "--views", folder]) == 2
    capsys.readouterr()


# ------------------------------------------------------------------------------------------------------- the shared header --
def _host(tmp_path):
    """tests/cpp/tsdf_unfuse_host.cpp as a stand-alone host program under the address and undefined-behaviour sanitizers (a plain
    build where the toolchain has none)."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path / "tsdf_unfuse_host")
    base = [cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "tsdf_unfuse_host.cpp"), "-o", exe]
    if subprocess.run(base[:1] + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + base[1:], capture_output=True).returncode != 0:
        subprocess.check_call(base)
    return exe


# sum, weight, (sum_b, sum_g, sum_r, colour weight), the updates (confirmed, q, (B, G, R)) -> k, kc, Q, B, G, R, fits, colour fits
# and, where both fit, the cell behind the down-date.  Every expectation is written out by hand from the contract.
W20 = 1 << 20
CELLS = [
    # the one view of a cell leaves: everything returns to zero
    ((-300, 1, (10, 20, 30, 1), [(1, -300, (10, 20, 30))]), (1, 1, -300, 10, 20, 30, 1, 1), (0, 0, 0, 0, 0, 0)),
    # a FREE view leaves a cell with a CONFIRMED one: the colour cell is not touched
    ((1024 - 5, 2, (9, 8, 7, 1), [(0, 1024, (0, 0, 0))]), (1, 0, 1024, 0, 0, 0, 1, 1), (-5, 1, 9, 8, 7, 1)),
    # two of three views
    ((1024 + 100 - 1024, 3, (255, 0, 100, 2), [(0, 1024, (0, 0, 0)), (1, -1024, (255, 0, 50))]), (2, 1, 0, 255, 0, 50, 1, 1), (100, 1, 0, 0, 50, 1)),
    # weight 0 is hit; more views than the weight
    ((0, 0, (0, 0, 0, 0), [(0, 1024, (0, 0, 0))]), (1, 0, 1024, 0, 0, 0, 0, 0), None),
    ((2048, 2, (0, 0, 0, 0), [(0, 1024, (0, 0, 0))] * 3), (3, 0, 3072, 0, 0, 0, 0, 0), None),
    # a full weight, whatever is asked
    ((0, W20, (0, 0, 0, 0), [(1, 0, (0, 0, 0))]), (1, 1, 0, 0, 0, 0, 0, 0), None),
    ((5, W20 - 1, (0, 0, 0, 1), [(1, 5, (0, 0, 0))]), (1, 1, 5, 0, 0, 0, 1, 1), (0, W20 - 2, 0, 0, 0, 0)),
    # weight 1, sum 1024, a CONFIRMED q = 0 view: the emptied cell would keep a sum
    ((1024, 1, (1, 1, 1, 1), [(1, 0, (1, 1, 1))]), (1, 1, 0, 1, 1, 1, 0, 1), None),
    # |s'| == 1024 w' is the boundary, one more is out
    ((-2048, 3, (0, 0, 0, 0), [(0, 1024, (0, 0, 0))]), (1, 0, 1024, 0, 0, 0, 0, 1), None),
    ((-1024, 3, (0, 0, 0, 0), [(0, 1024, (0, 0, 0))]), (1, 0, 1024, 0, 0, 0, 1, 1), (-2048, 2, 0, 0, 0, 0)),
    # the extremes of the sum in 64 bits: sum -2^30 minus 64 x 1024 does not wrap
    ((-(1 << 30), W20 - 1, (0, 0, 0, 0), [(0, 1024, (0, 0, 0))] * 64), (64, 0, 65536, 0, 0, 0, 0, 1), None),
    # colour: too little weight; too little sum (one channel); weight left above the TSDF weight; a sum above 255 per update
    ((0, 2, (50, 50, 50, 0), [(1, 0, (1, 1, 1))]), (1, 1, 0, 1, 1, 1, 1, 0), None),
    ((0, 2, (50, 0, 50, 1), [(1, 0, (1, 1, 1))]), (1, 1, 0, 1, 1, 1, 1, 0), None),
    ((1024, 1, (0, 0, 0, 1), [(0, 1024, (0, 0, 0))]), (1, 0, 1024, 0, 0, 0, 1, 0), None),
    ((0, 2, (200, 200, 456, 2), [(1, 0, (200, 200, 200))]), (1, 1, 0, 200, 200, 200, 1, 0), None),
    ((0, 2, (200, 200, 455, 2), [(1, 0, (200, 200, 200))]), (1, 1, 0, 200, 200, 200, 1, 1), (0, 1, 0, 0, 255, 1)),
    # colour words that would wrap in 32 bits are decided in 64
    ((0, 2, (0xFFFFFFFF, 0, 0, 1), [(1, 0, (255, 0, 0))]), (1, 1, 0, 255, 0, 0, 1, 0), None),
]
TRUNCS = [((0.125, 0.0), 0.5), ((0.125, 0.25), 0.25), ((0.05, 0.0), float(F(4.0) * F(0.05))), ((0.125, -1.0), None), ((0.125, float("nan")), None),
          ((0.125, float("inf")), None)]


def test_host_header(tmp_path):
    exe = _host(tmp_path)
    blob = struct.pack("<I", len(TRUNCS)) + b"".join(struct.pack("<ff", *t) for t, _ in TRUNCS)
    blob += struct.pack("<I", len(CELLS))
    for (s, w, col, ups), _, _ in CELLS:
        blob += struct.pack("<iIIIIII", s, w, *col, len(ups))
        for confirmed, q, px in ups:
            blob += struct.pack("<IiBBBB", confirmed, q, *px, 0)
    (tmp_path / "in.bin").write_bytes(blob)
    r = subprocess.run([exe, str(tmp_path / "in.bin")], capture_output=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr.decode()[-3000:])
    rows = [ln.split() for ln in r.stdout.decode().splitlines()]
    got_t = [[int(x) for x in row[1:]] for row in rows if row[0] == "trunc"]
    assert len(got_t) == len(TRUNCS)
    for got, (_, want) in zip(got_t, TRUNCS):
        assert got == ([0, 0] if want is None else [1, int(np.array([want], F).view(np.uint32)[0])])
    it = iter(row for row in rows if row[0] != "trunc")
    for i, (_, want, after) in enumerate(CELLS):
        row = next(it)
        assert row[0] == "cell" and tuple(int(x) for x in row[1:]) == want, (i, row, want)
        if want[6] and want[7]:
            row = next(it)
            assert row[0] == "down" and tuple(int(x) for x in row[1:]) == after, (i, row, after)
        else:
            assert after is None
    assert next(it, None) is None
    # the table itself: the totals written out are those of the updates listed
    for (s, w, col, ups), want, after in CELLS:
        d = dict(k=len(ups), kc=sum(u[0] for u in ups), q=sum(u[1] for u in ups))
        assert (d["k"], d["kc"], d["q"]) == want[:3]
