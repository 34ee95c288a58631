"""The tracker's per-point arithmetic in register pairs (revo_amd/csrc/revo_track_px.h) on the host: the pair form k_track and
k_pair_info run against the scalar form it replaced, bit for bit.  No GPU."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pair_form_has_the_bits_of_the_scalar_form(tmp_path):
    """tests/cpp/track_px.cpp includes the header the kernels include and compares, on every field of the projected point, r0, r1,
    res, good, wr, the six Jacobian entries, the 27 normal-equation sums, the error terms and the retries' patch rule, samples
    and terms:
    - projections outside each of the four image bounds, exactly on them and one ulp to either side, Z = 0, -0 and negative Z;
    - res one and two ulps below, at and above edge_distance (filter on and off) and huber;
    - all-zero patches, patches with the no-edge value sqrtf(1e15f) in some and in all samples, a retry at every pixel offset of
      [-2, 2]^2 around candidate 0 (in the patch, and gathered);
    - 2 M seeded random points, poses, patches and thresholds.
    The hardware reciprocal is a host stand-in in both forms.  The program stops at the first differing bit and prints the case."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path / "track_px")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror",
                           os.path.join(ROOT, "tests", "cpp", "track_px.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[0] == "cases" and int(last[1]) > 2_000_000 and int(last[3]) == 0
    assert "random: 2000000 cases" in r.stdout and "bounds, Z = 0 and negative Z" in r.stdout
