"""Cost of the known-space calls (api.VoxelMap.observe_into / known_field_into / frontiers_into; revo_map_observe,
revo_map_known_field, revo_map_frontiers in include/revo_hip.h) on one GPU, written to profiles/map_seen_rates.txt.

The carving scene's map (tests/map_carve_cases.py: two dense 320x240 keyframes, 2 cm) and its four 320x240 depth views, in
boxes of 64^3, 128^3 and 256^3 cells around the map's median voxel; 3 warm-up calls, then median and best of `--reps` calls:

  1. revo_map_observe with 1 and with 8 views (the four views twice), images and volume on the device: a host clock around
     one call and the wait for the stream; beside it the bytes the call must move -- one byte per cell out, the depth images
     in -- and what share of the 8 TB/s HBM peak moving only those would be;
  2. revo_map_known_field beside revo_map_distance_field on the same boxes, device outputs: a host clock around one call
     and the wait for the stream for both (revo_map_distance_field_last_ms describes revo_map_distance_field alone), and
     beside it the plain field's device time through that call;
  3. revo_map_frontiers, volume and records on the device: a host clock around the counting call and the writing call.

    python profiles/map_seen_rates.py [--reps 10] [--commit TEXT] [--out profiles/map_seen_rates.txt]
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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_seen_rates.txt"))
    a = ap.parse_args()
    import torch
    from revo_amd import api, mapfile
    import map_carve_cases as cc
    lines = []

    def say(text=""):
        print(text)
        sys.stdout.flush()
        lines.append(text)

    def clock(fn):
        ms = []
        for r in range(3 + a.reps):
            t0 = time.perf_counter()
            fn()
            if r >= 3:
                ms.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ms)), min(ms)

    rec = cc.scene_records().astype(mapfile.RAW_DTYPE)
    cam = api.CameraPyr(cc.settings320())
    m = api.VoxelMap(cam, cc.VOXEL, dense=True)
    m.merge_raw(rec)
    centre = np.median(mapfile.key_axes(rec["key"]), 0).astype(np.int64)
    views = [(torch.from_numpy(np.ascontiguousarray(D)).cuda(), T, k) for D, T, k in cc.scene_views(False)]
    image_bytes = 320 * 240 * 4
    boxes = [("scene %d^3" % e, centre - e // 2, (e, e, e)) for e in (64, 128, 256)]
    say("Known space of the voxel map, one MI355X, source: %s" % a.commit)
    say("scene map: %d voxels of %g m; 320x240 depth views; median / best of %d calls after 3 warm-up calls" % (len(rec), m.voxel, a.reps))

    say("\n1. revo_map_observe, radius 1, images and volume on the device (host clock around the call and its wait)")
    say("%-14s %6s %10s %11s %11s %10s %10s %14s %12s" % ("box", "views", "cells", "free cells", "bytes moved", "median ms", "best ms", "Gcell-views/s", "bytes / peak"))
    volumes = {}
    d_info = torch.zeros(8, dtype=torch.int64, device="cuda")
    for name, lo, n in boxes:
        d = torch.empty(n, dtype=torch.uint8, device="cuda")
        cells = n[0] * n[1] * n[2]
        for nv in (1, 8):
            vs = (views + views)[:nv]
            med, best = clock(lambda: m.observe_into(d, vs, lo, d_info=d_info))
            nbytes = cells + nv * image_bytes
            say("%-14s %6d %10d %11d %11d %10.3f %10.3f %14.2f %11.2f%%" % (name, nv, cells, int(d_info[1].item()), nbytes, med, best, cells * nv / med / 1e6,
                                                                         100.0 * nbytes / (med * 1e-3) / HBM_PEAK))
        m.observe_into(d, views, lo)
        volumes[name] = d

    say("\n2. revo_map_known_field beside revo_map_distance_field (host clock around the call and its wait; device outputs)")
    say("%-14s %10s %8s %10s %12s %16s %16s %16s" % ("box", "cells", "solid", "unknown", "known free", "plain median ms", "known median ms", "plain device ms"))
    for name, lo, n in boxes:
        d2 = torch.empty(n, dtype=torch.int32, device="cuda")
        plain = clock(lambda: m.distance_field_into(d2, lo, n))[0]
        device = m.last_distance_field_ms()
        known = clock(lambda: m.known_field_into(d2, volumes[name], lo, n, d_info=d_info))[0]
        i = d_info.cpu().numpy()
        say("%-14s %10d %8d %10d %12d %16.3f %16.3f %16.3f" % (name, n[0] * n[1] * n[2], i[1], i[5], i[6], plain, known, device))

    say("\n3. revo_map_frontiers, volume and records on the device (host clock: the counting call, then the writing call)")
    say("%-14s %10s %12s %10s %10s" % ("box", "cells", "frontiers", "median ms", "best ms"))
    for name, lo, n in boxes:
        k = m.frontiers_into(None, volumes[name], lo)
        out = torch.empty((max(k, 1), 4), dtype=torch.int32, device="cuda")
        med, best = clock(lambda: (m.frontiers_into(None, volumes[name], lo), m.frontiers_into(out, volumes[name], lo)))
        say("%-14s %10d %12d %10.3f %10.3f" % (name, n[0] * n[1] * n[2], k, med, best))

    name, lo, n = boxes[0]
    want = mapfile.observe_records(cc.VOXEL, lo, n, cc.scene_views(False))[0]
    say("\nthe 64^3 volume holds the bytes of mapfile.observe_records: %s" % (volumes[name].cpu().numpy().tobytes() == want.tobytes()))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
