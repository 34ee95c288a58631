"""Surfaces for many sequences at once without a GPU: the exports and the layout of the new records from a compiled C
snippet; tests/cpp/align_stepper_host.cpp, which holds AlignStepper against align_loop_over on synthetic record sequences and checks
the host rules of revo_tsdf_many_host.h; the usage errors of run_tum's --streams-surface, decided before a device is opened; and the
refusal of --surface together with --streams, which stands."""
import ctypes as C
import os
import shutil
import subprocess

from revo_amd import _lib
from revo_amd.settings import MapTsdfFuseJob, MapTsdfTrackJob, MapTsdfTrackResult, MultiSurface, MultiSurfaceReport

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("revo_map_tsdf_fuse_many", "revo_map_tsdf_track_eval_many", "revo_map_tsdf_track_many", "revo_vo_multi_attach_surface", "revo_vo_multi_surface_last")


def test_exports_and_record_layouts(tmp_path):
    assert set(NEW) <= set(_lib.declared_symbols())
    L = _lib.lib()
    for name in NEW:
        assert hasattr(L, name), name
    recs = {"revo_map_tsdf_fuse_job": (MapTsdfFuseJob, 200), "revo_map_tsdf_track_job": (MapTsdfTrackJob, 200),
            "revo_map_tsdf_track_result": (MapTsdfTrackResult, 288), "revo_vo_multi_surface": (MultiSurface, 120),
            "revo_vo_multi_surface_report": (MultiSurfaceReport, 408)}
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


def test_the_stepper_is_the_loop(tmp_path):
    """tests/cpp/align_stepper_host.cpp: the loop and the stepper over the same record sequences (convergence at the first step, the
    iteration limit, LOST at the first pivot and after some steps, a flags-bit-0 record) give identical poses, iteration counts,
    statuses and evaluations; with the host sanitizers where the toolchain has them."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path / "align_stepper_host")
    base = [cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "align_stepper_host.cpp"), "-o", exe]
    if subprocess.run(base[:1] + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + base[1:], capture_output=True).returncode != 0:
        subprocess.check_call(base)
    r = subprocess.run([exe], capture_output=True, timeout=300)
    out = r.stdout.decode()
    assert r.returncode == 0, (out[-3000:], r.stderr.decode()[-3000:])
    lines = out.splitlines()
    assert lines[-1] == "ok" and "FAILED" not in out
    want = {"converged at the first step": (0, 1, 2), "the iteration limit": (1, 4, 5), "lost at the first pivot": (2, 0, 2), "lost after two steps": (2, 2, 4),
            "a record without an evaluation": (2, 0, 2), "converged after three steps": (0, 3, 4)}
    for name, (status, its, evals) in want.items():
        assert "%s: status %d iterations %d evaluations %d" % (name, status, its, evals) in lines, name


def test_run_tum_streams_surface_usage_errors(capsys):
    """The option rules of run_tum --streams-surface are decided before any file is read or a device is opened; --surface together with
    --streams is refused as before."""
    from revo_amd import run_tum
    base = ["settings.yaml", "dataset.yaml"]
    for extra in (["--map", "0.02", "--streams-surface", "s.ply"],                                    # without --streams
                  ["--streams", "2", "--streams-surface", "s.ply"],                                   # without --map
                  ["--map", "0.02", "--streams", "2", "--streams-surface"],                           # without a file name
                  ["--map", "0.02", "--streams", "2", "--streams-surface", "--streams-surface-track"],
                  ["--map", "0.02", "--streams", "2", "--streams-surface-track"],                     # without --streams-surface
                  ["--map", "0.02", "--streams", "2", "--streams-surface", "s.ply", "--surface-box", "0", "0", "0", "0", "4", "4"],
                  ["--map", "0.02", "--streams", "2", "--streams-surface", "s.ply", "--surface-box", "0", "0", "0", "4", "4"],
                  ["--map", "0.02", "--streams", "2", "--streams-surface", "s.ply", "--surface-trunc", "0"],
                  ["--map", "0.02", "--streams", "2", "--streams-surface", "s.ply", "--surface-min-weight", "x"],
                  ["--map", "0.02", "--streams", "2", "--streams-surface", "s.ply", "--surface", "t.ply"],  # both forms
                  ["--map", "0.02", "--surface", "s.ply", "--streams", "2"],                          # the sequential form with --streams: as before
                  ["--map", "0.02", "--surface", "s.ply", "--surface-track", "--streams", "2"]):
        assert run_tum.main(base + extra) == 2, extra
    assert "--streams-surface" in capsys.readouterr().out
