"""Batched exact unfuse and the streams' surface windows without a GPU: the exports and the layout of the new records
from a compiled C snippet; mapfile.tsdf_unfuse_many_records against per-job tsdf_unfuse_records on the shared cases of
map_unfuse_cases.py, refused jobs among fitting ones; the usage errors of run_tum's --streams-surface-window, decided before a device is
opened, with --surface-window together with --streams refused as before; tests/cpp/surface_ring_host.cpp, the window's policy."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from revo_amd import _lib, mapfile
from revo_amd.settings import MapTsdfFuseJob, MapTsdfUnfuseJob, MapTsdfUnfuseResult, MultiSurfaceWindowReport

import map_unfuse_cases as uc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("revo_map_tsdf_unfuse_many", "revo_vo_multi_surface_window", "revo_vo_multi_surface_window_last")


def test_exports_and_record_layouts(tmp_path):
    assert set(NEW) <= set(_lib.declared_symbols())
    L = _lib.lib()
    for name in NEW:
        assert hasattr(L, name), name
    assert L.revo_map_tsdf_unfuse_many(None, 1, None, None, 0) == -1 and L.revo_vo_multi_surface_window(None, 0, 1) == -1  # no device needed
    assert L.revo_vo_multi_surface_window_last(None, 0, None) == -1
    recs = {"revo_map_tsdf_unfuse_job": (MapTsdfUnfuseJob, 192), "revo_map_tsdf_unfuse_result": (MapTsdfUnfuseResult, 80),
            "revo_vo_multi_surface_window_report": (MultiSurfaceWindowReport, 104)}
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
        assert int(got[cname]) == size == C.sizeof(cls), cname
        end = 0
        for f, _t in cls._fields_:
            assert int(got["%s.%s" % (cname, f)]) == getattr(cls, f).offset == end, (cname, f)  # in order, no padding holes
            end += getattr(cls, f).size
        assert end == size, cname
    # the unfuse job is the fuse job without color_info: the members they share have one meaning and one order
    assert [f for f, _ in MapTsdfUnfuseJob._fields_] == [f for f, _ in MapTsdfFuseJob._fields_ if f != "color_info"]


def _jobs():
    """Jobs of one call from the shared cases: every case that takes one view out (it fits), and every refusal of one view, with and
    without the colour volume, the refused ones between the fitting ones.  -> [(job, refused)]."""
    fit = []
    for name, c in uc.cases().items():
        if len(c["removed"]) != 1:
            continue
        cells, col = uc.fused(name, "all")
        views, bgr = uc.pick(c, c["removed"])
        for color in (True, False):
            fit.append((dict(cells=cells, color=col if color else None, lo=c["lo"], voxel=uc.V, view=views[0], trunc=c["trunc"],
                             bgr=bgr[0] if color else None), False))
    bad = []
    for name, r in uc.refusals().items():
        if len(r["views"]) != 1:
            continue
        for color in (True, False):
            if (color and r.get("tsdf_only")) or (not color and r.get("color_only") and r.get("tsdf_fits", True)):
                continue
            bad.append((dict(cells=r["cells"], color=r["color"] if color else None, lo=r["lo"], voxel=uc.V, view=r["views"][0], trunc=r["trunc"],
                             bgr=r["bgr"][0] if color else None), True))
    assert len(fit) >= 4 and len(bad) >= 4
    out = [bad[0]]  # a refused job first, one last, the others spread between the fitting ones
    gap = max(1, len(fit) // max(1, len(bad) - 2))
    rest = bad[1:-1]
    for i, f in enumerate(fit):
        out.append(f)
        if i % gap == gap - 1 and rest:
            out.append(rest.pop(0))
    return out + rest + [bad[-1]]


def test_unfuse_many_records_is_the_single_contract_per_job():
    jobs = _jobs()
    got = mapfile.tsdf_unfuse_many_records([j for j, _ in jobs])
    assert len(got) == len(jobs)
    n_refused, n_updates = 0, 0
    for i, ((j, refused), g) in enumerate(zip(jobs, got)):
        args = (j["cells"], j["color"], j["lo"], j["voxel"], [j["view"]], j["trunc"])
        kw = dict(bgr=None if j["color"] is None else [j["bgr"]])
        if refused:
            n_refused += 1
            with pytest.raises(mapfile.TsdfUnfuseRefused) as e:
                mapfile.tsdf_unfuse_records(*args, **kw)
            assert g["status"] == -1 and g["info"] == e.value.info and g["info"]["misfits"] == e.value.misfits > 0, i
            assert g["info"]["updates"] == 0 and g["info"]["color_updates"] == 0
            assert g["cells"] is j["cells"] and g["color"] is j["color"], i  # no byte of a refused job's volumes changed
            # view_info is still the fuse's
            assert g["counts"] == mapfile.tsdf_records(j["voxel"], j["lo"], np.shape(j["cells"]), [j["view"]], j["trunc"])[2][0], i
        else:
            cells, col, info, counts = mapfile.tsdf_unfuse_records(*args, **kw)
            assert g["status"] == 0 and g["info"] == info and g["counts"] == counts[0] and info["misfits"] == 0, i
            n_updates += info["updates"]
            assert g["cells"].tobytes() == cells.tobytes() and (col is None) == (g["color"] is None), i
            assert col is None or g["color"].tobytes() == col.tobytes(), i
    assert 0 < n_refused < len(jobs) and n_updates > 0
    # neither the order nor the other jobs show in a job's result
    back = mapfile.tsdf_unfuse_many_records([j for j, _ in jobs[::-1]])[::-1]
    for g, b in zip(got, back):
        assert g["status"] == b["status"] and g["info"] == b["info"] and g["counts"] == b["counts"] and g["cells"].tobytes() == b["cells"].tobytes()
    # the call's own argument errors are of the whole call
    j0 = jobs[1][0]
    for bad in ([], [j0] * 1025, [dict(j0, color=None, bgr=np.zeros((12, 16, 3), np.uint8))], [dict(j0, trunc=-1.0)]):
        with pytest.raises(ValueError):
            mapfile.tsdf_unfuse_many_records(bad)


def test_run_tum_streams_surface_window_usage_errors(capsys):
    """The option rules of --streams-surface-window are decided before any file is read or a device is opened."""
    from revo_amd import run_tum
    base = ["settings.yaml", "dataset.yaml", "--map", "0.02", "--streams", "2"]
    for extra in (["--streams-surface-window", "2"],                                   # without --streams-surface
                  ["--streams-surface", "s.ply", "--streams-surface-window"],           # without a number
                  ["--streams-surface", "s.ply", "--streams-surface-window", "x"],
                  ["--streams-surface", "s.ply", "--streams-surface-window", "0"],
                  ["--streams-surface", "s.ply", "--streams-surface-window", "-1"],
                  ["--streams-surface", "s.ply", "--streams-surface-window", "1025"]):
        assert run_tum.main(base + extra) == 2, extra
    assert "--streams-surface-window" in capsys.readouterr().out
    # without --streams or --map the surface's own rules speak
    assert run_tum.main(["settings.yaml", "dataset.yaml", "--map", "0.02", "--streams-surface", "s.ply", "--streams-surface-window", "2"]) == 2
    assert run_tum.main(["settings.yaml", "dataset.yaml", "--streams", "2", "--streams-surface", "s.ply", "--streams-surface-window", "2"]) == 2
    capsys.readouterr()
    # the sequential window together with --streams keeps its message
    assert run_tum.main(base + ["--surface", "s.ply", "--surface-window", "2"]) == 2
    assert "--surface-window is not supported together with --streams" in capsys.readouterr().out


def test_the_window_policy(tmp_path):
    """tests/cpp/surface_ring_host.cpp: revo_surface_ring.h against a plain queue -- the window at 1, at N and at N + 1, a ring that
    wraps, skipped keyframes, the largest window; with the host sanitizers where the toolchain has them."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path / "surface_ring_host")
    base = [cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "surface_ring_host.cpp"), "-o", exe]
    if subprocess.run(base[:1] + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + base[1:], capture_output=True).returncode != 0:
        subprocess.check_call(base)
    r = subprocess.run([exe], capture_output=True, timeout=300)
    out = r.stdout.decode()
    assert r.returncode == 0, (out[-3000:], r.stderr.decode()[-3000:])
    lines = out.splitlines()
    assert lines[-1] == "ok" and "FAILED" not in out
    for want in ("window 1, one keyframe: window 1 fused 1 held 1 evictions 0 last evicted -1",
                 "window 1, two keyframes: window 1 fused 2 held 1 evictions 1 last evicted 0",
                 "window 4, at the window: window 4 fused 4 held 4 evictions 0 last evicted -1",
                 "window 4, one above: window 4 fused 5 held 4 evictions 1 last evicted 0",
                 "window 4, the ring wraps: window 4 fused 23 held 4 evictions 19 last evicted 18",
                 "window 3, every third keyframe skipped: window 3 fused 14 held 3 evictions 11 last evicted 15",
                 "the largest window: window 1024 fused 1030 held 1024 evictions 6 last evicted 5"):
        assert want in lines, want
