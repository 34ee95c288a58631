"""Cost of the information matrices of tracked poses (revo_batch_pair_info / k_pair_info) on one GPU.

  1. One batched call for 32 pairs at 640x480, level 0, at the poses of the grid's own device records, against the only way
     there was before: 32 revo_optimizer_eval calls (a launch, a wait and a host round trip each).  Wall time around a
     synchronised call, warm-up, then median and best of `--reps`.
  2. The pipelined step (api.Pipeline, 32 pairs, the default depth) with and without the information in the after-grid slot of
     every step, interleaved: wall time per step over runs of `--steps` steps, median and best of `--reps` runs each.

    python profiles/pair_info_rates.py [--reps 20] [--steps 16]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _stats(v):
    return float(np.median(v)), float(np.min(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=16)
    a = ap.parse_args()
    import torch
    from revo_amd import api, synth
    from revo_amd.settings import ImgPyramidSettings, OptimizerSettings, TrackerSettings
    s = ImgPyramidSettings.scaled(640, 480, 4, hist_patch=(20, 10, 5, 0, 0, 0))
    cam = api.CameraPyr(s)
    trk = api.TrackerNew(TrackerSettings(), s, cam)
    opt = api.Optimizer(OptimizerSettings(), cam)
    N = 32
    pairs = synth.make_pairs(range(900, 900 + N), s)
    bgr = torch.from_numpy(np.stack([p[k][0] for p in pairs for k in ("ref", "curr")])).cuda()
    dep = torch.from_numpy(np.stack([p[k][1] for p in pairs for k in ("ref", "curr")])).cuda()
    d_res = torch.zeros(N * 96, dtype=torch.uint8, device="cuda")
    d_info = torch.zeros(N * 192, dtype=torch.uint8, device="cuda")

    print("1. information of %d pairs, 640x480 level 0 (ms, wall, median / best of %d)" % (N, a.reps))
    bt = api.BatchTracker(cam, N)
    bt.track(bgr.data_ptr(), dep.data_ptr(), d_res.data_ptr())
    bt.sync()
    res = api.results_from_buffer(d_res.cpu().numpy().tobytes(), N)
    t_batch = []
    for k in range(3 + a.reps):
        t0 = time.perf_counter()
        bt.pair_info(d_results=d_res.data_ptr(), lvl=0, d_info=d_info.data_ptr())
        bt.sync()
        if k >= 3:
            t_batch.append((time.perf_counter() - t0) * 1e3)
    pyrs = []
    for p in pairs:
        ref = api.ImgPyramidRGBD(s, cam, *p["ref"])
        cur = api.ImgPyramidRGBD(s, cam, *p["curr"])
        ref.makeKeyframe()
        pyrs.append((ref, cur))
    t_eval = []
    for k in range(3 + a.reps):
        t0 = time.perf_counter()
        for (ref, cur), r in zip(pyrs, res):
            opt.evalAt(ref, cur, r["R"], r["T"], 0)
        if k >= 3:
            t_eval.append((time.perf_counter() - t0) * 1e3)
    print("   one revo_batch_pair_info call      %8.3f / %8.3f" % _stats(t_batch))
    print("   %d revo_optimizer_eval calls       %8.3f / %8.3f" % ((N,) + _stats(t_eval)))
    del pyrs

    print("2. pipelined step of %d pairs (ms per step, wall, runs of %d steps, median / best of %d runs)" % (N, a.steps, a.reps))
    pipe = api.Pipeline(cam, N)
    depth = pipe.info()["batches"]
    d_r = [torch.zeros(N * 96, dtype=torch.uint8, device="cuda") for _ in range(depth)]
    d_i = [torch.zeros(N * 192, dtype=torch.uint8, device="cuda") for _ in range(depth)]

    def run(with_info):
        tickets = []
        t0 = time.perf_counter()
        for k in range(a.steps):
            if k >= depth:
                pipe.wait(tickets[k - depth])
            t, stream = pipe.submit(bgr.data_ptr(), dep.data_ptr(), d_r[k % depth].data_ptr())
            if with_info:
                pipe.pair_info(t, stream, d_i[k % depth].data_ptr(), d_results=d_r[k % depth].data_ptr(), lvl=0)
            tickets.append(t)
        pipe.drain()
        return (time.perf_counter() - t0) * 1e3 / a.steps

    times = {False: [], True: []}
    try:
        for k in range(2 + a.reps):
            for w in (False, True):
                ms = run(w)
                if k >= 2:
                    times[w].append(ms)
    finally:
        pipe.close()
    print("   without information                %8.3f / %8.3f" % _stats(times[False]))
    print("   with information (after-grid slot) %8.3f / %8.3f" % _stats(times[True]))
    _ = trk


if __name__ == "__main__":
    main()
