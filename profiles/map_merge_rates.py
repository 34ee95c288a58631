"""Cost of moving the voxel map as data (revo_map_export_raw / revo_map_merge_raw / revo_map_merge) on one GPU.

Two dense 1 cm maps of K 640x480 keyframes each (poses a few centimetres apart, so the halves share most voxels).  Timed with
the wall clock around calls closed by info() (waits for the map), 3 warm-up rounds, median and best of `runs`:

  merge        revo_map_merge(dst, src): dst holds the first half, src the second, straight from src's table
  merge_raw d  revo_map_merge_raw from src's records in device memory (always the checked path: the device looks at them)
  merge_raw h  revo_map_merge_raw from src's records in host memory (validated on the host, uploaded, fused path)
  export h/d   revo_map_export_raw of the merged map into host memory (sorted) / device memory
  integrate    the alternative a map without merge has: integrate the second half's K keyframes again
               (revo_map_integrate_many, one launch)

Every timed merge starts from a fresh copy of the first half (built by a merge_raw that is not timed) in a table large enough
that nothing grows.  No rate is asserted anywhere.

    python profiles/map_merge_rates.py [--keyframes 4] [--runs 20] [--voxel 0.01]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=4)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--voxel", type=float, default=0.01)
    a = ap.parse_args()
    import torch
    from revo_amd import api, synth
    from revo_amd.settings import ImgPyramidSettings
    s = ImgPyramidSettings.scaled(640, 480, 4, hist_patch=(20, 10, 5, 0, 0, 0))
    cam = api.CameraPyr(s)
    K = a.keyframes
    pyrs = [api.ImgPyramidRGBD(s, cam, *synth.make_pair(1300 + i, s)["ref"]) for i in range(2 * K)]
    Ts = [synth.se3_exp(np.array([0.03 * i, 0.01 * i, 0, 0, 0.01 * i, 0])).astype(np.float32) for i in range(2 * K)]
    big = 1 << 23

    def fresh(idx, initial=big):
        m = api.VoxelMap(cam, a.voxel, dense=True, initial_voxels=initial)
        m.integrate_many([pyrs[i] for i in idx], [Ts[i] for i in idx])
        m.info()
        return m

    first, second = fresh(range(K)), fresh(range(K, 2 * K), 1 << 16)  # merge reads every slot of src's table: grown, not pre-sized
    rec_first, rec_second = first.export_raw(), second.export_raw()
    d_second = torch.from_numpy(rec_second.view(np.uint8).copy()).cuda()
    whole = fresh(range(2 * K))
    want = whole.export_raw().tobytes()
    print("640x480 dense, voxel %g m, %d + %d keyframes: %d + %d voxels, %d in the union; median / best of %d, ms"
          % (a.voxel, K, K, len(rec_first), len(rec_second), whole.info()["voxels"], a.runs))

    def copy_of_first():
        m = api.VoxelMap(cam, a.voxel, dense=True, initial_voxels=big)
        m.merge_raw(rec_first, 0, K)
        m.info()
        return m

    def timed(name, body, nbytes=None, check=True):
        ts = []
        for r in range(a.runs + 3):
            m = copy_of_first()
            t0 = time.perf_counter()
            body(m)
            m.info()
            dt = time.perf_counter() - t0
            if r >= 3:
                ts.append(dt)
            if check and r == 0 and m.export_raw().tobytes() != want:
                raise SystemExit("%s: the merged map is not the map of all keyframes" % name)
            m.close()
        rate = ("  %6.1f GB/s of records" % (nbytes / np.median(ts) / 1e9)) if nbytes else ""
        print("%-12s %9.3f %9.3f%s" % (name, 1e3 * np.median(ts), 1e3 * min(ts), rate))
        sys.stdout.flush()

    nb = 64 * len(rec_second)
    timed("merge", lambda m: m.merge(second), nb)
    timed("merge_raw d", lambda m: m.merge_raw(d_second, 0, K), nb)
    timed("merge_raw h", lambda m: m.merge_raw(rec_second, 0, K), nb)
    timed("integrate", lambda m: m.integrate_many(pyrs[K:], Ts[K:]))
    d_out = torch.empty(64 * (len(rec_first) + len(rec_second)), dtype=torch.uint8, device="cuda")
    nw = 64 * whole.info()["voxels"]
    for name, body in (("export h", lambda: whole.export_raw()), ("export d", lambda: whole.export_raw_into(d_out))):
        ts = []
        for r in range(a.runs + 3):
            t0 = time.perf_counter()
            body()
            if r >= 3:
                ts.append(time.perf_counter() - t0)
        print("%-12s %9.3f %9.3f  %6.1f GB/s of records" % (name, 1e3 * np.median(ts), 1e3 * min(ts), nw / np.median(ts) / 1e9))


if __name__ == "__main__":
    main()
