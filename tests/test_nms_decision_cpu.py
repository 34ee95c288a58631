"""The per-pixel decision of Canny's non-maximum suppression (revo_amd/csrc/revo_nms_px.h) on the host: the threshold form
k_canny_nms4 runs -- one comparison of the magnitude against the largest value it must exceed -- against the reference form
(two neighbour comparisons and the two thresholds), on the candidate and the strong bit.  No GPU."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_threshold_form_decides_like_the_reference(tmp_path):
    """tests/cpp/nms_decision.cpp includes the header the kernel includes and compares the two forms over
    - every 3x3 neighbourhood whose neighbours come from {0, 1, 2, m - 1, m, m + 1, 2 080 800}, for centres m from 0 to the
      largest |grad|^2, one gradient per direction class (both sign pairs on the diagonals), threshold pairs 0 / low < high /
      low == high / low > high placed around m;
    - every gradient of [-1020, 1020]^2: the direction class itself (both sides of the two tan 22.5 boundaries at every |dx|,
      all sign combinations) and the decision on two tie-rich neighbourhoods, with low < high and low > high;
    - 2 M seeded random cases;
    - the order in which the kernel pushes four decisions into a bitmap nibble."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path / "nms_decision")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "nms_decision.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[0] == "cases" and int(last[1]) > 300_000_000 and int(last[3]) == 0
    assert "random: 2000000 cases" in r.stdout and "2041 x 2041 directions" in r.stdout
