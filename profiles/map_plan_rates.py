"""Cost of planning through the map (api.VoxelMap.plan_into / plan_paths_into; revo_map_plan, revo_map_plan_paths in
include/revo_hip.h) on one GPU, written to profiles/map_plan_rates.txt.

Device time and rounds of one call through revo_map_plan_last (HIP events on the tracker stream from the first kernel to the end
of the last one, the host's looks between the groups of rounds included; device field and output), 3 warm-up calls, then median
and best of `--reps` calls, and the host's clock around the same calls:

  1. the carving scene's map (tests/map_carve_cases.py: two dense 320x240 keyframes, 2 cm): the fields of profiles/
     map_field_rates.py's boxes of 64^3, 128^3 and 256^3 cells around its median voxel at r2 = 1 and 9 from one seed (the free
     cell nearest the box's centre), and a 256^3 box that holds no voxel; beside each a call whose only seed lies outside the
     box -- the passes over the cells and one group of rounds in which no tile runs -- so that the rounds' share shows;
  2. revo_map_plan_paths for 2^16 starts spread over the scene 256^3 box (cost field and outputs on the device): a host clock
     around one call that ends in a wait;
  3. revo_amd.mapfile.plan_records (numpy) and scipy.sparse.csgraph.dijkstra on the scene 64^3 box, on this machine's CPU.

    python profiles/map_plan_rates.py [--reps 20] [--commit TEXT] [--out profiles/map_plan_rates.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def nearest_free(d2, r2):
    """The free cell (relative) nearest the box's centre, looked for in the 32^3 cells around it."""
    c = np.asarray(d2.shape) // 2
    free = np.argwhere(d2[c[0] - 16:c[0] + 16, c[1] - 16:c[1] + 16, c[2] - 16:c[2] + 16] >= r2) + (c - 16)
    return free[np.argmin(((free - c) ** 2).sum(1))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_plan_rates.txt"))
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
    say("Planning through the voxel map, one MI355X, source: %s" % a.commit)
    say("scene map: %d voxels of %g m; per call: device time (HIP events) and host time, median / best of %d calls after 3 warm-up calls" % (len(rec), m.voxel, a.reps))
    say("\n1. revo_map_plan, device field and output, one seed at the free cell nearest the box's centre; `idle`: the same call with its seed outside the box")
    say("%-14s %3s %10s %10s %10s %7s %10s %9s %10s %10s %12s" % ("box", "r2", "cells", "reachable", "max cost", "rounds", "median ms", "best ms", "host ms", "idle ms", "Mcells / s"))
    d_info = torch.zeros(8, dtype=torch.int64, device="cuda")
    keep = {}
    for name, lo, n in [("scene %d^3" % e, centre - e // 2, (e, e, e)) for e in (64, 128, 256)] + [("empty 256^3", np.array([5000, 5000, 5000]), (256, 256, 256))]:
        d_d2 = torch.empty(n, dtype=torch.int32, device="cuda")
        m.distance_field_into(d_d2, lo, n)
        d2 = d_d2.cpu().numpy().view(np.uint32)
        d_cost = torch.empty(n, dtype=torch.int32, device="cuda")
        for r2 in (1, 9):
            seed = [tuple(int(v) for v in nearest_free(d2, r2) + lo)]
            ms, host, rounds = [], [], 0
            for r in range(3 + a.reps):
                t0 = time.perf_counter()
                m.plan_into(d_cost, d_d2, lo, n, seed, r2, d_info=d_info)
                dt = time.perf_counter() - t0
                t, rounds = m.last_plan()
                if r >= 3:
                    ms.append(t)
                    host.append(dt * 1e3)
            i = d_info.cpu().numpy()
            idle = []
            for r in range(3 + a.reps):
                m.plan_into(d_cost, d_d2, lo, n, [tuple(int(v) for v in lo - 1)], r2)
                if r >= 3:
                    idle.append(m.last_plan()[0])
            med = float(np.median(ms))
            say("%-14s %3d %10d %10d %10d %7d %10.3f %9.3f %10.3f %10.3f %12.1f" % (name, r2, i[0], i[2], i[3], rounds, med, min(ms), float(np.median(host)),
                                                                                  float(np.median(idle)), i[0] / med / 1e3))
            if r2 == 1:
                m.plan_into(d_cost, d_d2, lo, n, seed, r2)
                keep[name] = (d_cost.clone(), lo, d2, seed)

    say("\n2. revo_map_plan_paths, 2^16 starts over the scene 256^3 box at r2 = 1, max_len 512 (cost field and outputs on the device)")
    d_cost, lo, _, _ = keep["scene 256^3"]
    K, ML = 1 << 16, 512
    rng = np.random.default_rng(1)
    starts = rng.integers(0, 256, (K, 3)) + lo
    d_cells = torch.empty((K, ML, 3), dtype=torch.int32, device="cuda")
    d_paths = torch.zeros((K, 4), dtype=torch.int32, device="cuda")
    ts = []
    for r in range(2 + 5):
        t0 = time.perf_counter()
        m.plan_paths_into(d_cells, d_paths, d_cost, lo, starts, ML)
        ts.append(time.perf_counter() - t0)
    p = d_paths.cpu().numpy()
    dt = float(np.median(ts[2:]))
    say("%d starts (%d reached, %d unreachable, %d truncated), %d path cells, longest %d: %.3f ms per call (host clock, median of 5), %.1f Mcells / s" %
        (K, int((p[:, 1] == 0).sum()), int((p[:, 1] == 1).sum()), int((p[:, 1] == 3).sum()), int(p[:, 0].sum()), int(p[:, 0].max()), dt * 1e3, p[:, 0].sum() / dt / 1e6))

    say("\n3. the scene 64^3 box at r2 = 1 on the host CPU")
    d_c, lo, d2, seed = keep["scene 64^3"]
    n = d2.shape
    t0 = time.perf_counter()
    want, info = mapfile.plan_records(d2, lo, n, seed, 1)
    dt = time.perf_counter() - t0
    say("mapfile.plan_records (numpy sweeps): %.1f ms (%d reachable cells, largest cost %d); the device's cost field holds the same bytes: %s" %
        (dt * 1e3, info["reachable"], info["max_cost"], d_c.cpu().numpy().view(np.uint32).tobytes() == want.tobytes()))
    try:
        import scipy.sparse as sp
        from scipy.sparse.csgraph import dijkstra
        t0 = time.perf_counter()
        free = d2 >= 1
        idx = np.arange(free.size).reshape(n)
        rows, cols, w = [], [], []
        for dx, dy, dz in mapfile.PLAN_MOVES:
            sa = tuple(slice(max(0, -d), n[k] - max(0, d)) for k, d in enumerate((dx, dy, dz)))
            sb = tuple(slice(max(0, d), n[k] - max(0, -d)) for k, d in enumerate((dx, dy, dz)))
            ok = free[sa] & free[sb]
            rows.append(idx[sa][ok])
            cols.append(idx[sb][ok])
            w.append(np.full(int(ok.sum()), 2 + (dx != 0) + (dy != 0) + (dz != 0), np.float64))
        g = sp.csr_matrix((np.concatenate(w), (np.concatenate(rows), np.concatenate(cols))), shape=(free.size, free.size))
        t1 = time.perf_counter()
        d = dijkstra(g, directed=True, indices=[int(idx[tuple(np.asarray(seed[0]) - lo)])], min_only=True).reshape(n)
        t2 = time.perf_counter()
        same = np.where(np.isfinite(d) & free, d, float(mapfile.PLAN_NONE)).astype(np.uint32).tobytes() == want.tobytes()
        say("scipy.sparse.csgraph.dijkstra: %.1f ms for the graph, %.1f ms for the search; the same costs: %s" % ((t1 - t0) * 1e3, (t2 - t1) * 1e3, same))
    except ImportError:
        say("scipy is not installed")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
