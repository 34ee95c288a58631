"""Cost of the batched surface calls (revo_map_tsdf_fuse_many, revo_map_tsdf_track_eval_many, revo_map_tsdf_track_many; include/revo_hip.h,
DESIGN 31) on one GPU, written to profiles/multi_surface_rates.txt.

DESIGN 28's protocol: 3 warm-up calls, then the median of `--reps` calls with the range, a host clock around the call and its wait,
everything in device memory.  8 and 32 jobs, each on its own 128^3 TSDF and colour volume around the carving scene's median voxel
(2 cm voxels), 320x240 frames: the scene's four views, job j taking view j % 4.  The yardstick is the single calls, run in the same
process on the same inputs: as many accumulating revo_map_tsdf_fuse_color calls, as many revo_map_tsdf_track_eval calls, as many
revo_map_tsdf_track loops (from DESIGN 29's 2-voxel / 2-degree start `tr2`, axis j % 3).  The batched results are checked against
the single calls' bytes once, outside the clock.

    python profiles/multi_surface_rates.py [--reps 10] [--size 128] [--commit TEXT] [--out profiles/multi_surface_rates.txt]
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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multi_surface_rates.txt"))
    a = ap.parse_args()
    import torch
    from revo_amd import api, mapfile
    import map_carve_cases as cc
    import map_tsdf_track_cases as kc
    lines = []

    def say(text=""):
        print(text)
        sys.stdout.flush()
        lines.append(text)

    def clock(fn, reps=a.reps):
        ms = []
        for r in range(3 + reps):
            t0 = time.perf_counter()
            fn()
            if r >= 3:
                ms.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))

    rec = cc.scene_records().astype(mapfile.RAW_DTYPE)
    s = cc.settings320()
    cam = api.CameraPyr(s)
    m = api.VoxelMap(cam, cc.VOXEL, dense=True)
    e = a.size
    lo, n = tuple(int(x) for x in np.median(mapfile.key_axes(rec["key"]), 0).astype(np.int64) - e // 2), (e, e, e)
    frames = cc.scene_frames()[0]
    views = [(torch.from_numpy(np.ascontiguousarray(D)).cuda(), T, k, torch.from_numpy(np.ascontiguousarray(frames[i][0])).cuda())
             for i, (D, T, k) in enumerate(cc.scene_views(False))]
    k6 = cc.intrinsics320()
    trunc = float(mapfile.tsdf_trunc(cc.VOXEL))
    centre = ((np.asarray(lo, np.float64) + e / 2.0) * float(np.float32(cc.VOXEL))).astype(np.float32)
    truth = np.asarray(views[0][1], np.float32)

    def start(axis):  # DESIGN 29's tr2: turned by -2 degrees about the axis through the box's middle and moved by 2 voxel edges
        both = kc.about(truth, centre, axis, -2.0).astype(np.float64)
        both[(axis + 1) % 3, 3] -= 2.0 * cc.VOXEL
        return both.astype(np.float32)

    say("Batched surface calls against the single calls, one MI355X, source: %s" % a.commit)
    say("scene: 320x240 views, voxels of %g m, trunc %g m, every job its own %d^3 TSDF and colour volume; median (min .. max) of %d calls"
        % (cc.VOXEL, trunc, e, a.reps))
    say("after 3 warm-up calls, a host clock around the call and its wait, everything in device memory")
    ok = True
    for J in (8, 32):
        vols = [(torch.zeros(n + (2,), dtype=torch.int32, device="cuda"), torch.zeros(n + (4,), dtype=torch.int32, device="cuda")) for _ in range(J)]
        for j, (t, c) in enumerate(vols):  # every volume holds the four views: the model the tracking runs against
            m.fuse_into(t, views, lo, d_color=c)
        fuse_jobs = [dict(d_tsdf=t, d_color=c, lo=lo, view=views[j % 4]) for j, (t, c) in enumerate(vols)]

        def fuse_many():
            m.fuse_many_into(fuse_jobs)

        def fuse_single():
            for j, (t, c) in enumerate(vols):
                m.fuse_into(t, [views[j % 4]], lo, accumulate=True, wait=False, d_color=c)
            m.sync()

        frame = (views[0][0], k6[:4], k6[4:])
        poses = [start(j % 3) for j in range(J)]
        eval_jobs = [dict(tsdf=t, lo=lo, trunc=trunc, frame=frame, poses=poses[j], centre=centre) for j, (t, _) in enumerate(vols)]
        loop_jobs = [dict(tsdf=t, lo=lo, trunc=trunc, frame=frame, T_init=poses[j], centre=centre) for j, (t, _) in enumerate(vols)]
        d_out = torch.zeros(J * 208, dtype=torch.uint8, device="cuda")

        def eval_many():
            m.surface_track_eval_many(eval_jobs, d_out=d_out)
            m.sync()

        def eval_single():
            for j, (t, _) in enumerate(vols):
                m.surface_track_eval(t, lo, trunc, frame, poses[j], centre=centre, d_out=d_out[208 * j:208 * (j + 1)])
            m.sync()

        rounds = [0]

        def loop_many():
            rounds[0] = m.surface_track_many(loop_jobs)[1]

        def loop_single():
            return [m.surface_track(t, lo, trunc, frame, poses[j], centre=centre) for j, (t, _) in enumerate(vols)]

        # fuse first (it changes the volumes: the clocks of both forms run on volumes that keep growing in weight, as a sequence's do)
        rows = [("fuse_many, %d jobs" % J, clock(fuse_many)), ("%d accumulating fuse_color calls" % J, clock(fuse_single))]
        eval_many()
        got = d_out.cpu().numpy().tobytes()
        eval_single()
        ok = ok and got == d_out.cpu().numpy().tobytes()
        rows += [("track_eval_many, %d jobs, 1 pose each" % J, clock(eval_many)), ("%d track_eval calls" % J, clock(eval_single))]
        many, single = m.surface_track_many(loop_jobs)[0], loop_single()
        ok = ok and all(g["T"].tobytes() == w["T"].tobytes() and bytes(g["info"]) == bytes(w["info"]) and g["iterations"] == w["iterations"] and g["status"] == w["status"]
                        for g, w in zip(many, single))
        rows += [("track_many, %d jobs" % J, clock(loop_many)), ("%d track loops" % J, clock(loop_single))]
        say("\n%d jobs" % J)
        say("%-44s %10s %20s" % ("call", "ms", "min .. max"))
        for name, t in rows:
            say("%-44s %10.3f %9.3f .. %7.3f" % (name, t[0], t[1], t[2]))
        say("single / batched: fuse %.2f, track_eval %.2f, track %.2f; rounds of track_many: %d; iterations per job: %s; statuses: %s"
            % (rows[1][1][0] / rows[0][1][0], rows[3][1][0] / rows[2][1][0], rows[5][1][0] / rows[4][1][0], rounds[0],
               sorted(set(w["iterations"] for w in single)), sorted(set(w["status"] for w in single))))
        del vols, fuse_jobs, eval_jobs, loop_jobs
        torch.cuda.empty_cache()
    say("\nthe batched calls gave the single calls' bytes: %s" % ok)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    m.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
