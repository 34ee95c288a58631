"""Cost of the tracker's exact-sums mode (revo_ctx_set_exact_sums), default and exact alternating in one process.

  * k_track on the bench workload: 640x480, 4 levels, 32 pairs per batch (revo_batch_time_tracker: tracker grids alone);
  * single-pair trackFrames latency (api.TrackerNew.trackFrames, pyramids built beforehand);
  * revo_vo frames/s on one sequence (vo.REVO.push, the sequential stream);
  * revo_vo_multi frames/s at S = 32 (vo.MultiREVO.run);
  * the kernels' VGPRs / scratch / occupancy, from the compiler's resource remarks (hipcc -Rpass-analysis=kernel-resource-usage).

Each measurement is repeated --reps times, the two modes alternating, and reported as median [min, max].

    python profiles/exact_sums_rates.py [--reps 5] [--frames 40]
"""
import argparse
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def resources():
    """k_track's resource remarks (a compile of revo_track.hip for gfx950 to /dev/null)."""
    src = os.path.join(ROOT, "revo_amd", "csrc")
    cmd = [os.environ.get("HIPCC", "hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
           "-mllvm", "-disable-machine-licm", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
           "revo_track.hip", "-o", os.devnull]
    txt = subprocess.run(cmd, cwd=src, capture_output=True, text=True).stderr
    out, name = [], None
    for ln in txt.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            name = m.group(1)
            continue
        if name and "k_track" in name and "gate" not in name:
            m = re.search(r"(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", ln)
            if m:
                out.append((name, m.group(1), int(m.group(2))))
    rows = {}
    for name, k, v in out:
        t = re.search(r"k_trackILb(\d)ELb(\d)E", name)
        key = ("single" if t.group(1) == "1" else "batch") + ("/exact" if t.group(2) == "1" else "/default")
        rows.setdefault(key, {})[k.split(" ")[0]] = v
    return rows


def stat(xs):
    xs = sorted(xs)
    return "%.4g [%.4g, %.4g]" % (xs[len(xs) // 2], xs[0], xs[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=40)
    a = ap.parse_args()
    print("k_track resources (gfx950):")
    for k, v in sorted(resources().items()):
        print("  %-15s VGPRs %3d  AGPRs %d  scratch %d B/lane  occupancy %d waves/SIMD"
              % (k, v.get("VGPRs", -1), v.get("AGPRs", 0), v.get("ScratchSize", -1), v.get("Occupancy", -1)))
    import torch
    from revo_amd import api, synth, vo
    from revo_amd.settings import ImgPyramidSettings, TrackerSettings
    s = ImgPyramidSettings.scaled(640, 480, 4, hist_patch=(20, 10, 5, 0, 0, 0))
    pairs = synth.make_pairs(range(32), s)  # the bench's seeds
    bgr = torch.from_numpy(np.stack([p[k][0] for p in pairs for k in ("ref", "curr")])).cuda()
    dep = torch.from_numpy(np.stack([p[k][1] for p in pairs for k in ("ref", "curr")])).cuda()
    seq = [(f[0], f[1], f[2]) for f in synth.make_sequence(3, s, a.frames, max_t=0.01, max_rot_deg=0.4,
                                                           bias=[0.004, 0, 0, 0, np.deg2rad(0.5), 0], workers=8)]
    seqs = [[(f[0], f[1], f[2]) for f in synth.make_sequence(40 + k, s, a.frames, max_t=0.01, max_rot_deg=0.4,
                                                             bias=[0.003, 0, 0, 0, np.deg2rad(0.4), 0], workers=8)]
            for k in range(8)]
    res = {m: {"track_ms": [], "single_ms": [], "vo_fps": [], "multi_fps": []} for m in ("default", "exact")}
    evals = {}
    for rep in range(a.reps):
        for mode in (("default", "exact") if rep % 2 == 0 else ("exact", "default")):
            ex = mode == "exact"
            cam = api.CameraPyr(s, exact_sums=ex)
            trk = api.TrackerNew(TrackerSettings(), s, cam)
            bt = api.BatchTracker(cam, 32)
            d_res = torch.zeros(32 * 96, dtype=torch.uint8, device="cuda")
            bt.build(bgr.data_ptr(), dep.data_ptr())
            bt.sync()
            res[mode]["track_ms"].append(bt.time_tracker(d_res.data_ptr(), reps=20))
            recs = api.results_from_buffer(d_res.cpu().numpy().tobytes(), 32)
            evals[mode] = sum(int(r["evals"][:4].sum()) for r in recs)
            ref = api.ImgPyramidRGBD(s, cam, *pairs[0]["ref"])
            cur = api.ImgPyramidRGBD(s, cam, *pairs[0]["curr"])
            ref.makeKeyframe()
            trk.trackFrames(np.eye(3), np.zeros(3), ref, cur)
            torch.cuda.synchronize()
            t = []
            for _ in range(20):
                t0 = time.perf_counter()
                trk.trackFrames(np.eye(3), np.zeros(3), ref, cur)
                t.append(time.perf_counter() - t0)
            res[mode]["single_ms"].append(1e3 * float(np.median(t)))
            g = vo.REVO(s, cameraPyr=cam)
            t0 = time.perf_counter()
            for f in seq:
                g.push(*f)
            res[mode]["vo_fps"].append(len(seq) / (time.perf_counter() - t0))
            m = vo.MultiREVO(s, 32, exact_sums=ex)
            t0 = time.perf_counter()
            out = m.run([seqs[k % 8] for k in range(32)])
            res[mode]["multi_fps"].append(sum(len(o) for o in out) / (time.perf_counter() - t0))
            del m, g, bt, trk, cam
    print("\n%d repetitions, modes alternating; median [min, max]" % a.reps)
    labels = [("track_ms", "k_track, 32 pairs 640x480x4 (ms per grid)"), ("single_ms", "single-pair trackFrames (ms)"),
              ("vo_fps", "revo_vo, one sequence (frames/s)"), ("multi_fps", "revo_vo_multi, S = 32 (frames/s)")]
    for k, lab in labels:
        d, e = res["default"][k], res["exact"][k]
        print("  %-44s default %-28s exact %-28s exact/default %.3f" % (lab, stat(d), stat(e), np.median(e) / np.median(d)))
    print("  LM evaluations of the 32 bench pairs: default %d, exact %d" % (evals["default"], evals["exact"]))


if __name__ == "__main__":
    main()
