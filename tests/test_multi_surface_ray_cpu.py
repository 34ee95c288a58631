"""Batched TSDF ray casts without a GPU: the export and the layout of the job record from a compiled C snippet;
mapfile.tsdf_raycast_many_records against per-job tsdf_raycast_records over the table of map_tsdf_ray_cases.py, jobs that share a
volume among them; the usage errors of run_tum's --streams-surface-views, decided before a device is opened, with --surface-views
together with --streams refused as before; tests/cpp/tsdf_ray_many_host.cpp, the planning rules and the overlap check."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from revo_amd import _lib, mapfile
from revo_amd.settings import MapDfBox, MapTsdfRayJob, MapTsdfRayParams

import map_tsdf_ray_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_export_and_job_layout(tmp_path):
    assert "revo_map_tsdf_raycast_many" in _lib.declared_symbols()
    assert "revo_*" in open(os.path.join(ROOT, "revo_amd", "csrc", "revo_hip.ver")).read()  # the version script exports the header's names
    L = _lib.lib()
    assert hasattr(L, "revo_map_tsdf_raycast_many")
    assert L.revo_map_tsdf_raycast_many(None, 1, None) == -1  # no device needed
    cname, cls, size = "revo_map_tsdf_ray_job", MapTsdfRayJob, 120
    body = '  printf("%s %%zu\\n", sizeof(%s));\n' % (cname, cname)
    for f, _t in cls._fields_:
        body += '  printf("%s.%s %%zu\\n", offsetof(%s, %s));\n' % (cname, f, cname, f)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "revo_hip.h"\nint main(void) {\n%s  return 0;\n}\n' % body)
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    got = dict(ln.split(None, 1) for ln in subprocess.run([str(exe)], capture_output=True, check=True).stdout.decode().splitlines())
    assert int(got[cname]) == size == C.sizeof(cls)
    end = 0
    for f, _t in cls._fields_:
        assert int(got["%s.%s" % (cname, f)]) == getattr(cls, f).offset == end, f  # in order, no padding holes
        end += getattr(cls, f).size
    assert end == size
    want = dict(map=0, box=8, prm=32, tsdf=48, color=56, n_views=64, reserved=68, views=72, depth=80, normal=88, bgr=96, hits=104, info=112)
    assert {f: getattr(cls, f).offset for f, _ in cls._fields_} == want  # the offsets the header documents
    header = open(os.path.join(ROOT, "include", "revo_hip.h")).read()
    record = header[header.index("typedef struct revo_map_tsdf_ray_job"):header.index("} revo_map_tsdf_ray_job;")]
    for f, off in want.items():
        assert "offset %3d:" % off in record, (f, off)
    assert C.sizeof(MapDfBox) == 24 and C.sizeof(MapTsdfRayParams) == 16


def _jobs():
    """Every case of the table as a job, then jobs that share a case's volume: other views, another min_weight, another step."""
    cases = rc.cases()
    jobs = [dict(cells=c["cells"], color=c["color"], lo=c["lo"], voxel=rc.V, views=c["views"], step=c["step"], min_weight=c["min_weight"],
                 max_steps=c["max_steps"]) for c in cases.values()]
    c = cases["tilted plane 20x20x20"]
    jobs.append(dict(cells=c["cells"], color=None, lo=c["lo"], voxel=rc.V, views=c["views"][::-1], min_weight=2))
    jobs.append(dict(cells=c["cells"], color=c["color"], lo=c["lo"], voxel=rc.V, views=c["views"][:1], step=0.05))
    return jobs


def test_raycast_many_records_is_the_single_contract_per_job():
    jobs = _jobs()
    got = mapfile.tsdf_raycast_many_records(jobs)
    assert len(got) == len(jobs) and sum(g["info"]["hits"] for g in got) > 0
    assert jobs[-1]["cells"] is jobs[-2]["cells"]  # shared volumes are among them
    keys = ("depth", "normals", "bgr", "status", "samples", "colored")

    def same(a, b, what):
        assert a["hits"] == b["hits"] and a["info"] == b["info"], what
        for k in keys:
            for x, y in zip(a[k], b[k]):
                assert (x is None) == (y is None) and (x is None or x.tobytes() == y.tobytes()), (what, k)

    for i, (j, g) in enumerate(zip(jobs, got)):
        alone = mapfile.tsdf_raycast_records(j["cells"], j.get("color"), j["lo"], j["voxel"], j["views"], j.get("step"), j.get("min_weight", 1),
                                             j.get("max_steps", 4096))
        same(g, alone, i)
    # neither the order nor the other jobs show in a job's result
    part = jobs[-6:]
    back = mapfile.tsdf_raycast_many_records(part[::-1])[::-1]
    for i, (g, b) in enumerate(zip(got[-6:], back)):
        same(g, b, ("reversed", i))
    # the call's own argument errors are of the whole call
    j0 = jobs[0]
    small = dict(j0, views=[(rc.I4, (8.5, 8.5, 0.0, 0.0, rc.ZMIN, rc.ZMAX), (1, 1))] * 64)
    mapfile.tsdf_raycast_many_records([small] * 2)
    for bad in ([], [j0] * 1025, [small] * 65, [dict(j0, views=[])], [dict(j0, views=list(small["views"]) + [small["views"][0]])], [j0, dict(j0, step=-1.0)],
                [j0, dict(j0, max_steps=(1 << 20) + 1)], [j0, dict(j0, views=[(rc.I4, rc.KC, (0, 12))])],
                [j0, dict(j0, color=np.zeros((1, 1, 1), mapfile.TSDF_COLOR_DTYPE))]):
        with pytest.raises(ValueError):
            mapfile.tsdf_raycast_many_records(bad)


def test_run_tum_streams_surface_views_usage_errors(capsys):
    """The option rules of --streams-surface-views are decided before any file is read or a device is opened."""
    from revo_amd import run_tum
    base = ["settings.yaml", "dataset.yaml", "--map", "0.02", "--streams", "2"]
    for extra in (["--streams-surface-views", "views"],                                                    # without --streams-surface
                  ["--streams-surface", "s.ply", "--streams-surface-views"],                               # without a folder
                  ["--streams-surface", "s.ply", "--streams-surface-views", "--exact-sums"],
                  ["--streams-surface", "s.ply", "--streams-surface-views-every", "2"],                    # without --streams-surface-views
                  ["--streams-surface", "s.ply", "--streams-surface-views", "views", "--streams-surface-views-every"],
                  ["--streams-surface", "s.ply", "--streams-surface-views", "views", "--streams-surface-views-every", "x"],
                  ["--streams-surface", "s.ply", "--streams-surface-views", "views", "--streams-surface-views-every", "0"]):
        assert run_tum.main(base + extra) == 2, extra
    out = capsys.readouterr().out
    assert "--streams-surface-views ray-casts every stream's TSDF surface: it needs --streams-surface FILE.ply" in out
    assert "--streams-surface-views needs a folder name" in out and "--streams-surface-views-every needs" in out
    # without --streams or --map the surface's own rules speak
    views = ["--streams-surface", "s.ply", "--streams-surface-views", "views"]
    assert run_tum.main(["settings.yaml", "dataset.yaml", "--map", "0.02"] + views) == 2
    assert run_tum.main(["settings.yaml", "dataset.yaml", "--streams", "2"] + views) == 2
    capsys.readouterr()
    # the sequential views together with --streams stay refused
    assert run_tum.main(base + ["--surface", "s.ply", "--surface-views", "views"]) == 2
    assert "--surface is not supported together with --streams" in capsys.readouterr().out
    assert run_tum.main(base + ["--streams-surface", "s.ply", "--surface-views", "views"]) == 2
    assert "--surface-views ray-casts the TSDF surface: it needs --surface FILE.ply" in capsys.readouterr().out
    assert "--streams-surface-views DIR" in run_tum.__doc__
    assert run_tum.main([]) == 2 and "[--streams-surface-views DIR [--streams-surface-views-every K]]" in capsys.readouterr().out


def test_the_planning_rules_and_the_overlap_check(tmp_path):
    """tests/cpp/tsdf_ray_many_host.cpp: revo_tsdf_ray_many_host.h against plain loops -- the distinct volumes, the masks' offsets, the
    first_block sums and the view rows for 1 job, 1024 jobs, every job sharing one volume and no two sharing; touching ranges
    accepted, one shared byte refused; with the host sanitizers where the toolchain has them."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path / "tsdf_ray_many_host")
    base = [cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "tsdf_ray_many_host.cpp"), "-o", exe]
    if subprocess.run(base[:1] + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + base[1:], capture_output=True).returncode != 0:
        subprocess.check_call(base)
    r = subprocess.run([exe], capture_output=True, timeout=300)
    out = r.stdout.decode()
    assert r.returncode == 0, (out[-3000:], r.stderr.decode()[-3000:])
    lines = out.splitlines()
    assert lines[-1] == "ok" and "FAILED" not in out
    for want in ("one job: jobs 1 distinct volumes 1 mask bytes 256 mask blocks 6 views 64",
                 "1024 jobs, no two sharing: jobs 1024 distinct volumes 1024 mask bytes 262144 mask blocks 1036 views 2560",
                 "1024 jobs sharing one volume: jobs 1024 distinct volumes 1 mask bytes 512 mask blocks 8192 views 4096",
                 "mixed sharing: jobs 8 distinct volumes 5 mask bytes 1280 mask blocks 5 views 79",
                 "overlap: touching accepted, one shared byte refused"):
        assert want in lines, want
