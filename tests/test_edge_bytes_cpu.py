"""The bitmap forms behind the lazily produced byte edge planes (revo_amd/csrc/revo_edge_bits.h: the bit -> byte expansion of
k_edge_bytes and k_fill's condition on the finer level's edge bitmap) on the host, against the byte forms.  No GPU."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bitmap_forms_equal_byte_forms(tmp_path):
    """tests/cpp/edge_bytes.cpp includes the header the kernels include and compares, on seeded random bitmaps of the widths
    80, 96, 100 and 160 (with garbage in the unused bits of a partial last word):
    - every 16-pixel group of the expansion with the plane's bytes, at densities from empty to full -- width 100 takes the
      form whose groups wrap into the next row;
    - fill-in of a coarse level from the finer level's bitmap with fill-in from its byte plane, pixel by pixel, with the gate
      forced closed (nothing may be added), forced open (something must be) and left to the tile counts.
    The program prints the first differing cases and exits non-zero on any."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path / "edge_bytes")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "edge_bytes.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[0] == "cases" and int(last[1]) > 1_000_000 and int(last[3]) == 0
    assert "expand:" in r.stdout and "fill:" in r.stdout
