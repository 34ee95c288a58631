"""Aggregate rate of many sequential-VO streams through one revo_vo_multi handle (vo.MultiREVO), 640x480, 4 levels.

Eight seeded synthetic sequences are rendered once into page-locked memory, laid out [frame][sequence] so that the frames
of one submit lie back to back (stream s plays sequence s % 8).  For every S the handle runs S streams for the whole
length of the sequences, t+1's frames submitted before step t like MultiREVO.run; the clock runs from the first submit to
the last pose.  The single-stream vo.REVO rate (IO thread + consumer loop, the bench's sequential stream) is measured in
the same process on the same frames.  Depth goes in as f32 metres and as raw u16 (TUM's on-disk format, 1.5 instead of
2.1 MB a frame over PCIe; the conversion is fused into the build), each against the single stream with the same input.

    python profiles/multi_stream_rates.py [--frames 48] [--streams 1,4,8,16,32,64] [--reps 3] [--depth f32,u16] [--workers 8]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--streams", default="1,4,8,16,32,64")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--depth", default="f32,u16")
    ap.add_argument("--workers", type=int, default=8, help="renderer processes (1: render in this process)")
    a = ap.parse_args()
    import torch
    from revo_amd import synth, vo
    from revo_amd.settings import ImgPyramidSettings
    s = ImgPyramidSettings.scaled(640, 480, 4, hist_patch=(20, 10, 5, 0, 0, 0))
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

    dep16 = torch.empty((F, NB, H, W), dtype=torch.int16).pin_memory().numpy().view(np.uint16)
    dep16[...] = np.clip(dep * 5000.0, 0, 65535).astype(np.uint16)  # how TUM stores depth (iowrapperRGBD.cpp:326-327)
    DSF = 5000.0

    def single(depth):
        D = dep16 if depth == "u16" else dep
        dsf = DSF if depth == "u16" else None
        g = vo.REVO(s, depth_scale_factor=dsf)
        frames = [(bgr[t, 0], D[t, 0], ts[t, 0]) for t in range(F)]
        g.run(frames)  # warm-up (frame sets, kernels)
        best = 0.0
        for _ in range(a.reps):
            g = vo.REVO(s, cameraPyr=g.camPyr, depth_scale_factor=dsf)
            t0 = time.perf_counter()
            g.run(frames)
            best = max(best, F / (time.perf_counter() - t0))
        return best

    def multi(S, m, D):
        for st in range(S):
            m.reset(st)
        frames_at = lambda t: [(st, bgr[t, st % NB], D[t, st % NB], ts[t, st % NB]) for st in range(S)]
        t_next, steps, kf_steps, poses = 0, 0, 0, 0
        t0 = time.perf_counter()
        while poses < S * F:
            while t_next < F and all(m.pending(st) < m.max_queue for st in range(S)):
                m.submit(frames_at(t_next))
                t_next += 1
            busy = sum(1 for st in range(S) if m.pending(st) > 0)
            res = m.step()
            steps += 1
            poses += len(res)
            kf_steps += 1 if len(res) < busy else 0  # some stream's vote asked for a keyframe: its re-track is owed
        dt = time.perf_counter() - t0
        return S * F / dt, dt / steps * 1e3, steps, kf_steps

    print("640x480 x 4 levels, %d frames per sequence, %d repetitions (best)" % (F, a.reps))
    for depth in a.depth.split(","):
        D = dep16 if depth == "u16" else dep
        r1 = single(depth)
        print("\n%s depth -- single-stream vo.REVO (IO thread): %.0f frames/s" % (depth, r1))
        print("%4s %12s %10s %8s %10s %8s" % ("S", "frames/s", "ms/step", "steps", "kf-steps", "x single"))
        for S in [int(x) for x in a.streams.split(",")]:
            m = vo.MultiREVO(s, S, depth_scale_factor=DSF if depth == "u16" else None)
            multi(S, m, D)  # warm-up: frame sets, past-cloud buffers
            best = None
            for _ in range(a.reps):
                r = multi(S, m, D)
                if best is None or r[0] > best[0]:
                    best = r
            print("%4d %12.0f %10.3f %8d %10d %8.2f" % (S, best[0], best[1], best[2], best[3], best[0] / r1))
            sys.stdout.flush()
            del m
        print("%s depth -- single-stream vo.REVO again: %.0f frames/s" % (depth, single(depth)))

if __name__ == "__main__":
    main()
