"""Cost of the voxel map's distance field (api.VoxelMap.distance_field_into / sample_into; revo_map_distance_field,
revo_map_df_sample in include/revo_hip.h) on one GPU, written to profiles/map_field_rates.txt.

Device time of one call through revo_map_distance_field_last_ms (HIP events on the tracker stream from the first memset to the
end of the last pass; device output), 3 warm-up calls, then median and best of `--reps` calls:

  1. the carving scene's map (tests/map_carve_cases.py: two dense 320x240 keyframes, 2 cm) in boxes of 64^3, 128^3 and 256^3
     cells around its median voxel, and a 256^3 box that holds no voxel; beside each the algorithmic bytes -- the bit volume
     plus 4 B read and 4 B written per cell and pass -- over the measured time, as a fraction of the 8 TB/s HBM peak;
  2. revo_map_df_sample for 2^20 points spread over the 256^3 box, field, points and output on the device: a host clock
     around `--reps` enqueued calls that end in a wait for the stream;
  3. revo_amd.mapfile.distance_field_records (numpy, this machine's CPU) on the 64^3 box.

    python profiles/map_field_rates.py [--reps 20] [--commit TEXT] [--out profiles/map_field_rates.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_field_rates.txt"))
    a = ap.parse_args()
    import torch
    from revo_amd import api, mapfile
    import map_carve_cases as cc
    lines = []

    def say(text=""):
        print(text)
        sys.stdout.flush()
        lines.append(text)

    rec = cc.scene_records().astype(mapfile.RAW_DTYPE)
    cam = api.CameraPyr(cc.settings320())
    m = api.VoxelMap(cam, cc.VOXEL, dense=True)
    m.merge_raw(rec)
    centre = np.median(mapfile.key_axes(rec["key"]), 0).astype(np.int64)
    say("The voxel map's distance field, one MI355X, source: %s" % a.commit)
    say("scene map: %d voxels of %g m in %d slots; device time per call, median / best of %d calls after 3 warm-up calls" %
        (len(rec), m.voxel, m.info()["capacity"], a.reps))
    say("\n1. revo_map_distance_field, device output (bytes: the bit volume + 8 B per cell and pass, three passes; peak 8 TB/s)")
    say("%-18s %10s %8s %8s %10s %10s %12s %10s %9s" % ("box", "cells", "solid", "max d2", "median ms", "best ms", "Gcells / s", "GB / s", "of peak"))
    per_cell = {}
    d_info = torch.zeros(8, dtype=torch.int64, device="cuda")
    fields = {}
    for name, lo, n in [("scene %d^3" % e, centre - e // 2, (e, e, e)) for e in (64, 128, 256)] + [("empty 256^3", np.array([5000, 5000, 5000]), (256, 256, 256))]:
        d = torch.empty(n, dtype=torch.int32, device="cuda")
        ms = []
        for r in range(3 + a.reps):
            m.distance_field_into(d, lo, n, d_info=d_info, wait=False)
            t = m.last_distance_field_ms()
            if r >= 3:
                ms.append(t)
        i = d_info.cpu().numpy()
        cells = n[0] * n[1] * n[2]
        nbytes = 4 * n[0] * n[1] * ((n[2] + 31) // 32) + 3 * 8 * cells
        med = float(np.median(ms))
        per_cell[name] = med / cells
        fields[name] = (d, lo)
        say("%-18s %10d %8d %8d %10.3f %10.3f %12.2f %10.1f %8.1f%%" % (name, cells, i[1], i[4], med, min(ms), cells / med / 1e6, nbytes / med / 1e6,
                                                                      100.0 * nbytes / (med * 1e-3) / HBM_PEAK))
    ratio = per_cell["empty 256^3"] / per_cell["scene 256^3"]
    say("empty 256^3 against scene 256^3, time per cell: %.2f x" % ratio)

    say("\n2. revo_map_df_sample, 2^20 points over and around the scene 256^3 box (field, points, output on the device)")
    d, lo = fields["scene 256^3"]
    N = 1 << 20
    rng = np.random.default_rng(1)
    p = rng.uniform((lo - 16) * m.voxel, (lo + 256 + 16) * m.voxel, (N, 3)).astype(np.float32)
    d_p = torch.from_numpy(p).cuda()
    d_o = torch.empty((N, 4), dtype=torch.float32, device="cuda")
    for r in range(3):
        m.sample_into(d_o, d, lo, d_p)
    t0 = time.perf_counter()
    for r in range(a.reps):
        m.sample_into(d_o, d, lo, d_p, wait=False)
    m.sync()
    dt = (time.perf_counter() - t0) / a.reps
    inside = int((d_o[:, 0] >= 0).sum().item())
    say("%d points (%d inside the box): %.3f ms per call (host clock over %d calls, then a wait), %.1f Mpoints / s" % (N, inside, dt * 1e3, a.reps, N / dt / 1e6))

    say("\n3. the numpy restatement (mapfile.distance_field_records) on the scene 64^3 box, on the host CPU")
    t0 = time.perf_counter()
    want, info = mapfile.distance_field_records(rec, centre - 32, (64, 64, 64))
    dt = time.perf_counter() - t0
    got = torch.empty((64, 64, 64), dtype=torch.int32, device="cuda")
    m.distance_field_into(got, centre - 32, (64, 64, 64))
    same = got.cpu().numpy().view(np.uint32).tobytes() == want.tobytes()
    say("%.1f ms (%d solid voxels, largest d2 %d); the device's field holds the same bytes: %s" % (dt * 1e3, info["solid"], info["max_d2"], same))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
