"""Cost of the batched unfuse (revo_map_tsdf_unfuse_many; include/revo_hip.h) on one GPU, written to
profiles/multi_unfuse_rates.txt.

DESIGN 31's protocol: 3 warm-up calls, then the median of `--reps` calls with the range, a host clock around the call and its wait,
everything in device memory.  8 and 32 jobs, each on its own 128^3 TSDF and colour volume around the carving scene's median voxel
(2 cm voxels) holding the scene's four views, 320x240 frames; job j takes view j % 4 out.  The yardstick is as many single
revo_map_tsdf_unfuse calls, run in the same process on the same inputs (that code is the parent commit's).  An unfuse changes the
volumes, so behind every clocked call the views are fused back, outside the clock.  Rows: unfuse_many with host results (its one
wait inside); unfuse_many only enqueued plus one stream wait; the single calls; the refused case (one cell of every job at the full
weight, so every job has one misfit and nothing is applied) in both forms.  The batched results are checked against the single
calls' bytes once, outside the clock.  Last, three short sequences through vo.MultiREVO with surfaces, with and without window=2:
the whole run's wall time, since a step's surface part is not isolated from the step.

    python profiles/multi_unfuse_rates.py [--reps 10] [--size 128] [--commit TEXT] [--out profiles/multi_unfuse_rates.txt]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multi_unfuse_rates.txt"))
    a = ap.parse_args()
    import torch
    from revo_amd import api, mapfile
    from revo_amd._lib import RevoError
    import map_carve_cases as cc
    lines = []

    def say(text=""):
        print(text)
        sys.stdout.flush()
        lines.append(text)

    def clock(fn, restore=None, reps=a.reps):
        ms = []
        for r in range(3 + reps):
            t0 = time.perf_counter()
            fn()
            if r >= 3:
                ms.append((time.perf_counter() - t0) * 1e3)
            if restore is not None:
                restore()
        return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))

    rec = cc.scene_records().astype(mapfile.RAW_DTYPE)
    cam = api.CameraPyr(cc.settings320())
    m = api.VoxelMap(cam, cc.VOXEL, dense=True)
    e = a.size
    lo, n = tuple(int(x) for x in np.median(mapfile.key_axes(rec["key"]), 0).astype(np.int64) - e // 2), (e, e, e)
    frames = cc.scene_frames()[0]
    views = [(torch.from_numpy(np.ascontiguousarray(D)).cuda(), T, k, torch.from_numpy(np.ascontiguousarray(frames[i][0])).cuda())
             for i, (D, T, k) in enumerate(cc.scene_views(False))]
    trunc = float(mapfile.tsdf_trunc(cc.VOXEL))

    say("Batched unfuse against the single calls, one MI355X, source: %s" % a.commit)
    say("scene: 320x240 views, voxels of %g m, trunc %g m, every job its own %d^3 TSDF and colour volume holding the four views; median (min .. max) of %d calls"
        % (cc.VOXEL, trunc, e, a.reps))
    say("after 3 warm-up calls, a host clock around the call and its wait, everything in device memory; the views are fused back outside the clock")
    ok = True
    for J in (8, 32):
        vols = [(torch.zeros(n + (2,), dtype=torch.int32, device="cuda"), torch.zeros(n + (4,), dtype=torch.int32, device="cuda")) for _ in range(J)]
        for t, c in vols:
            m.fuse_into(t, views, lo, d_color=c)
        jobs = [dict(d_tsdf=t, d_color=c, lo=lo, view=views[j % 4]) for j, (t, c) in enumerate(vols)]
        d_res = torch.zeros(20 * J, dtype=torch.int32, device="cuda")

        def put_back():
            m.fuse_many_into(jobs)

        def many_host():
            return m.unfuse_many_into(jobs, wait=True)

        def many_enqueued():
            m.unfuse_many_into(jobs, wait=False, d_results=d_res)
            m.sync()

        def single():
            for j, (t, c) in enumerate(vols):
                m.unfuse_into(t, [views[j % 4]], lo, d_color=c, wait=False)
            m.sync()

        def single_refused():
            for j, (t, c) in enumerate(vols):
                try:
                    m.unfuse_into(t, [views[j % 4]], lo, d_color=c, wait=False)
                except RevoError:
                    pass
            m.sync()

        # the bytes, once: the batched call on the volumes, the single calls on copies
        copies = [(t.clone(), c.clone()) for t, c in vols]
        res = many_host()
        for j, (t, c) in enumerate(copies):
            info = m.unfuse_into(t, [views[j % 4]], lo, d_color=c)
            ok = ok and res[j] == (info, 0) and bool((t == vols[j][0]).all()) and bool((c == vols[j][1]).all())
        del copies
        put_back()
        rows = [("unfuse_many, %d jobs, host results" % J, clock(many_host, put_back)),
                ("unfuse_many, %d jobs, enqueued + one wait" % J, clock(many_enqueued, put_back)),
                ("%d unfuse calls" % J, clock(single, put_back))]
        # the refused case: one cell that the job's view updates is at the full weight
        for j, (t, c) in enumerate(vols):
            alone = torch.zeros_like(t)
            m.fuse_into(alone, [views[j % 4][:3]], lo)
            hit = (alone[..., 1] > 0).nonzero()
            x, y, z = (int(v) for v in hit[len(hit) // 2])
            t[x, y, z, 1] = 1 << 20
            del alone
        torch.cuda.synchronize()
        res = many_host()
        ok = ok and all(s == -1 and i["misfits"] == 1 and i["updates"] == 0 for i, s in res)
        rows += [("unfuse_many, %d jobs, every job refused" % J, clock(many_host)), ("%d unfuse calls, every one refused" % J, clock(single_refused))]
        say("\n%d jobs" % J)
        say("%-48s %10s %20s" % ("call", "ms", "min .. max"))
        for name, t in rows:
            say("%-48s %10.3f %9.3f .. %7.3f" % (name, t[0], t[1], t[2]))
        say("single / batched: host results %.2f, enqueued %.2f, refused %.2f" % (rows[2][1][0] / rows[0][1][0], rows[2][1][0] / rows[1][1][0], rows[4][1][0] / rows[3][1][0]))
        del vols, jobs
        torch.cuda.empty_cache()
    say("\nthe batched calls gave the single calls' bytes and infos: %s" % ok)
    m.close()

    # the driver: three streams with surfaces, with and without a window of 2 -- whole runs, the surface part is not isolated
    try:
        from lm_settings_cases import S160
        from revo_amd import synth, vo
        from test_gpu_voxel_map import BIASES
        seqs = [[(f[0], f[1], f[2]) for f in synth.make_sequence(seed, S160, 70, max_t=0.01, max_rot_deg=0.4, bias=BIASES[b])] for seed, b in zip((41, 42, 43), (1, 0, 2))]
        say("\nvo.MultiREVO, 3 streams of 70 frames (160x120), a 32^3 colour surface per stream; wall time of run(), median (min .. max) of 5 after 1 warm-up")
        for window in (None, 2):
            ms, kfs, ev = [], 0, 0
            for r in range(6):
                mv = vo.MultiREVO(S160, 3, map_voxel=0.05, map_dense=True, surface=dict(lo=(-16, -16, 14), n=(32, 32, 32), **({} if window is None else {"window": window})))
                t0 = time.perf_counter()
                out = mv.run(seqs)
                if r >= 1:
                    ms.append((time.perf_counter() - t0) * 1e3)
                kfs = sum(sum(1 for _, kf in o if kf) for o in out)
                ev = sum(o.surface_evictions for o in out)
                for o in out:
                    o.map.close()
                del mv
            say("%-48s %10.3f %9.3f .. %7.3f   (%d keyframes, %d evictions)" % ("run(), window=%s" % window, np.median(ms), np.min(ms), np.max(ms), kfs, ev))
    except Exception as ex:  # the kernel rows above stand on their own
        say("\nthe driver rows were not measured: %r" % (ex,))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
