"""The per-lane search of the EDT row pass (revo_amd/csrc/revo_edt_px.h: four pixels per lane from aligned 16-byte windows) on
the host, against a brute-force min over the row, as integers.  No GPU."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_window_search_equals_brute_force(tmp_path):
    """tests/cpp/edt_px.cpp includes the header k_edt_rows includes, lays every row out as the kernel does ([pad INF][g2][pad INF]
    between guard words that would win every minimum if they were read) and compares all w minima and their roots with
    min_x' (x - x')^2 + g2(x'):
    - widths 4, 8, 12, 36, 80, 160, 640 and 2048;
    - all-INF rows; one finite column at x = 0, at x = w-1 and at each of the four positions of a quad; finite columns only in
      the first or only in the last quad (the search runs to d = w-1 and into the padding); column distances 0, 1 and 2047 and
      the fill's 0xffff -> INF rule;
    - 200 000 seeded random rows, from one finite column per row to all finite;
    - the root of every minimum seen is the correctly rounded one, from the estimate and from one ulp to either side of it;
    - the division-free group index for every operand pair of its range.
    The program prints the first differing case and exits non-zero on any."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path / "edt_px")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror",
                           os.path.join(ROOT, "tests", "cpp", "edt_px.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[0] == "cases" and int(last[1]) > 200_000 and int(last[3]) == 0
    assert "random: 200000 rows" in r.stdout and "edges of the layout" in r.stdout
    roots = [ln for ln in r.stdout.splitlines() if ln.startswith("roots:")][0].split()
    assert int(roots[1]) > 10_000  # distinct minima whose roots were checked
