"""Cost of the world-frame voxel map (api.VoxelMap, revo_map_* in include/revo_hip.h) on one GPU, 640x480.

  1. One integration: wall time of `reps` back-to-back VoxelMap.integrate calls of one 640x480 keyframe into a map that already
     holds its voxels (the steady state of overlapping keyframes), closed by info() (waits for the map), per call; and the first
     integration into an empty, pre-sized map.  Edge and dense clouds, voxel 1 cm and 5 cm.  Best and median of `runs`.
  2. Table growth: a dense 1 mm map is filled keyframe by keyframe (random poses, a few 10^5 new voxels each) from a small table;
     a call that grows the table (allocation, clearing, the rehash kernel, freeing the old table) is timed against the median
     call that does not.  Reported with the voxel count and the table sizes at that growth.
  3. revo_vo_multi frames/s at S streams (as profiles/multi_stream_rates.py: 8 seeded sequences, stream s plays s % 8, page-locked
     f32 depth): no map, an edge map per stream, a dense map per stream (MultiREVO-style attachment, the step's batched
     integration), and the obvious alternative -- generateColoredPcl per keyframe report plus a numpy fusion on the host
     (tests/voxel_map_ref.py's restatement; edges and dense).

    python profiles/voxel_map_rates.py [--frames 48] [--streams 8,32] [--runs 5] [--reps 20] [--workers 8]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--streams", default="8,32")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--workers", type=int, default=8)
    a = ap.parse_args()
    import torch
    from revo_amd import api, synth, vo
    from revo_amd.settings import ImgPyramidSettings
    import voxel_map_ref as ref
    s = ImgPyramidSettings.scaled(640, 480, 4, hist_patch=(20, 10, 5, 0, 0, 0))
    print("640x480 x 4 levels, one MI355X; best / median of %d runs" % a.runs)

    # ---- 1. one integration
    cam = api.CameraPyr(s)
    pair = synth.make_pair(1234, s)
    kf = api.ImgPyramidRGBD(s, cam, *pair["ref"])
    T = synth.se3_exp(np.array([0.3, -0.2, 0.5, 0.1, 0.2, -0.1])).astype(np.float32)
    print("\n1. one keyframe integration (%d back-to-back calls per run, map already holding its voxels; 'first' = into an "
          "empty pre-sized map)" % a.reps)
    print("%6s %6s %9s %12s %12s %12s %12s" % ("cloud", "voxel", "points", "voxels", "us best", "us median", "first us"))
    for dense in (False, True):
        for v in (0.01, 0.05):
            per, first = [], []
            for _ in range(a.runs):
                m = api.VoxelMap(cam, v, dense=dense, initial_voxels=1 << 20)
                m.info()
                t0 = time.perf_counter()
                m.integrate(kf, T)
                m.info()
                first.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                for _ in range(a.reps):
                    m.integrate(kf, T)
                m.info()
                per.append((time.perf_counter() - t0) / a.reps)
            i = m.info()
            print("%6s %6.2f %9d %12d %12.1f %12.1f %12.1f" % ("dense" if dense else "edges", v, i["points_integrated"] // (a.reps + 1),
                                                            i["voxels"], 1e6 * min(per), 1e6 * np.median(per), 1e6 * min(first)))
            sys.stdout.flush()

    # ---- 2. growth
    print("\n2. table growth (dense, 1 mm voxels, random poses): calls that grew the table vs the median call that did not")
    print("%12s %14s %12s %12s" % ("voxels", "slots", "growth ms", "plain ms"))
    rng = np.random.default_rng(7)
    m = api.VoxelMap(cam, 0.001, dense=True, initial_voxels=1 << 18, max_voxels=1 << 25)
    plain, grown = [], []
    while True:
        i0 = m.info()
        if i0["voxels"] > 9_000_000:
            break
        Tk = synth.se3_exp(np.concatenate([rng.uniform(-20, 20, 3), rng.uniform(-1, 1, 3)])).astype(np.float32)
        t0 = time.perf_counter()
        m.integrate(kf, Tk)
        i1 = m.info()
        dt = time.perf_counter() - t0
        if i1["rehashes"] > i0["rehashes"]:
            grown.append((i0["voxels"], i0["capacity"], i1["capacity"], dt))
        else:
            plain.append(dt)
    pm = np.median(plain)
    for vox, c0, c1, dt in grown:
        print("%12d %6d->%-7d %12.2f %12.2f" % (vox, c0 >> 20, c1 >> 20, 1e3 * dt, 1e3 * pm))
    print("(slots in 2^20; growth ms includes hipMalloc of the new table, its clearing, the rehash and hipFree of the old one)")
    del m

    # ---- 3. multi-stream rates
    NB, F, H, W = 8, a.frames, s.height, s.width
    biases = [[0.004, 0, 0, 0, np.deg2rad(0.5), 0], [0, 0.003, 0, np.deg2rad(0.4), 0, 0], [0.002, 0, 0.003, 0, 0, 0],
              [0, 0, 0, 0, np.deg2rad(0.8), 0], [0.004, 0.002, 0, 0, 0, np.deg2rad(0.3)], [0, 0, 0.004, 0, np.deg2rad(0.4), 0],
              [0.003, 0, 0, 0, 0, 0], [0, 0.002, 0.002, np.deg2rad(0.3), 0, 0]]
    bgr = torch.empty((F, NB, H, W, 3), dtype=torch.uint8).pin_memory().numpy()
    dep = torch.empty((F, NB, H, W), dtype=torch.float32).pin_memory().numpy()
    ts = np.zeros((F, NB))
    for k in range(NB):
        for t, f in enumerate(synth.make_sequence(900 + k, s, F, max_t=0.01, max_rot_deg=0.4, bias=biases[k], workers=a.workers)):
            bgr[t, k], dep[t, k], ts[t, k] = f[0], f[1], f[2]

    def multi(S, m, mode):
        maps = []
        host = []
        for st in range(S):
            m.reset(st)
            if mode in ("edges", "dense"):
                vm = api.VoxelMap(m.camPyr, 0.01, dense=mode == "dense", initial_voxels=1 << 20)
                m.attach_map(st, vm)
                maps.append(vm)
            if mode.startswith("host"):
                host.append(ref.VoxelMapRef(0.01))
        frames_at = lambda t: [(st, bgr[t, st % NB], dep[t, st % NB], ts[t, st % NB]) for st in range(S)]
        t_next, poses, kfs = 0, 0, 0
        t0 = time.perf_counter()
        while poses < S * F:
            while t_next < F and all(m.pending(st) < m.max_queue for st in range(S)):
                m.submit(frames_at(t_next))
                t_next += 1
            res = m.step()
            poses += len(res)
            for st, M, kf_, _ in res:
                if kf_:
                    kfs += 1
                    if host:
                        p, Tk = m.keyframe(st)
                        host[st].integrate_pcl(p.generateColoredPcl(0, mode == "host-dense"), Tk)
        for vm in maps:
            vm.info()  # the maps' last work is done
        if host:
            for h in host:
                h.points()  # the host map's extraction (the device map's runs lazily at extraction)
        dt = time.perf_counter() - t0
        return S * F / dt, kfs

    print("\n3. revo_vo_multi, %d frames per sequence, 1 cm voxels (frames/s, best of %d runs; median in brackets)" % (F, a.runs))
    modes = ["none", "edges", "dense", "host-edges", "host-dense"]
    print("%4s %10s" % ("S", "keyframes") + "".join("%22s" % x for x in modes))
    for S in [int(x) for x in a.streams.split(",")]:
        m = vo.MultiREVO(s, S)
        row = {}
        nkf = 0
        for mode in modes:
            multi(S, m, mode)  # warm-up
            rs = []
            for _ in range(a.runs if not mode.startswith("host") else max(1, a.runs // 2)):
                r, nkf = multi(S, m, mode)
                rs.append(r)
            row[mode] = (max(rs), float(np.median(rs)))
        print("%4d %10d" % (S, nkf) + "".join("%13.0f (%6.0f)" % row[x] for x in modes))
        sys.stdout.flush()
        del m


if __name__ == "__main__":
    main()
