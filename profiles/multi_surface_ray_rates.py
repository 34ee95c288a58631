"""Cost of the batched surface ray cast (revo_map_tsdf_raycast_many; include/revo_hip.h) on one GPU, written to
profiles/multi_surface_ray_rates.txt.

DESIGN 31's protocol: 3 warm-up calls, then the median of `--reps` calls with the range, a host clock around the call and its wait,
everything in device memory.  8 and 32 jobs, each on its own 128^3 TSDF and colour volume around the carving scene's median voxel
(2 cm voxels) holding the scene's four views; 320x240 views with depth, normals and colours, one view per job and eight views per
job (the scene's four poses and poses near them).  Then one volume seen from 256 poses: four jobs of 64 views that share it, against
four single calls of 64 views.  The yardstick is as many surface_raycast_into calls (revo_map_tsdf_raycast), only enqueued and
followed by one stream wait, in the same process on the same volumes.  The batched call is measured with both finishes: the trailing
launch that hands the counters over (the default) and the ticket per job (REVO_MAP_TSDF_RAY_MANY_TICKET=1).  Every batched result is
compared with the single calls' bytes once, outside the clock.

    python profiles/multi_surface_ray_rates.py [--reps 10] [--size 128] [--commit TEXT] [--out profiles/multi_surface_ray_rates.txt]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multi_surface_ray_rates.txt"))
    a = ap.parse_args()
    import torch
    from revo_amd import api, mapfile
    import map_carve_cases as cc
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
    h, w = int(s.height), int(s.width)
    rng = np.random.default_rng(34)

    def near(T):
        P = np.array(T, np.float32)
        P[:3, 3] += rng.uniform(-0.05, 0.05, 3).astype(np.float32)
        return P

    base = [np.array(v[1], np.float32) for v in views]

    def outputs(J, V):
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")  # noqa: E731
        return [dict(d_depth=z((V, h, w), torch.float32), d_normals=z((V, h, w, 3), torch.float32), d_bgr=z((V, h, w, 3), torch.uint8),
                     d_hits=z((64,), torch.int32)[:V], d_info=z((8,), torch.int64)) for _ in range(J)]

    def state(outs):
        torch.cuda.synchronize()
        return [tuple(o[k].cpu().numpy().tobytes() for k in ("d_depth", "d_normals", "d_bgr", "d_hits", "d_info")) for o in outs]

    def measure(title, vols, poses):
        """vols[j], poses[j]: job j's volumes and its poses -> the rows, and whether the bytes agree."""
        J, V = len(vols), len(poses[0])
        outs, ref = outputs(J, V), outputs(J, V)
        jobs = [dict(d_tsdf=t, d_color=c, lo=lo, poses=np.stack(p), **o) for (t, c), p, o in zip(vols, poses, outs)]

        def many():
            m.surface_raycast_many_into(jobs, wait=False)
            m.sync()

        def single(dst=outs):
            for (t, c), p, o in zip(vols, poses, dst):
                m.surface_raycast_into(o["d_depth"], t, lo, np.stack(p), d_normals=o["d_normals"], d_bgr=o["d_bgr"], d_color=c, d_hits=o["d_hits"],
                                       d_info=o["d_info"], wait=False)
            m.sync()

        single(ref)
        want = state(ref)
        same = True
        rows = []
        for ticket in ("0", "1"):
            os.environ["REVO_MAP_TSDF_RAY_MANY_TICKET"] = ticket
            for o in outs:
                for t_ in o.values():
                    t_.fill_(7)
            torch.cuda.synchronize()
            many()
            same = same and state(outs) == want
            rows.append(("raycast_many, %s" % ("a ticket per job" if ticket == "1" else "trailing launch"), clock(many)))
        os.environ["REVO_MAP_TSDF_RAY_MANY_TICKET"] = "0"
        rows.append(("%d raycast calls" % J, clock(single)))
        hits = int(sum(int(np.frombuffer(w_[4], np.int64)[1]) for w_ in want))
        say("\n%s: %d jobs x %d views, %d rays, %d hits" % (title, J, V, J * V * h * w, hits))
        say("%-48s %10s %20s" % ("call", "ms", "min .. max"))
        for name, t in rows:
            say("%-48s %10.3f %9.3f .. %7.3f" % (name, t[0], t[1], t[2]))
        say("single / batched: trailing launch %.2f, ticket %.2f; the batched bytes are the single calls': %s"
            % (rows[2][1][0] / rows[0][1][0], rows[2][1][0] / rows[1][1][0], same))
        return same

    say("Batched surface ray cast against the single calls, one MI355X, source: %s" % a.commit)
    say("scene: %dx%d views with depth, normals and colours, voxels of %g m, every volume %d^3 TSDF and colour cells holding the scene's four views"
        % (w, h, cc.VOXEL, e))
    say("median (min .. max) of %d calls after 3 warm-up calls, a host clock around the call and its wait, everything in device memory" % a.reps)
    ok = True
    for J in (8, 32):
        vols = [(torch.zeros(n + (2,), dtype=torch.int32, device="cuda"), torch.zeros(n + (4,), dtype=torch.int32, device="cuda")) for _ in range(J)]
        for t, c in vols:
            m.fuse_into(t, views, lo, d_color=c)
        ok = measure("own volumes", vols, [[base[j % 4]] for j in range(J)]) and ok
        ok = measure("own volumes", vols, [base + [near(base[(j + i) % 4]) for i in range(4)] for j in range(J)]) and ok
        if J == 8:
            poses = [near(base[i % 4]) for i in range(256)]
            ok = measure("one volume from 256 poses", [vols[0]] * 4, [poses[64 * k:64 * k + 64] for k in range(4)]) and ok
        del vols
        torch.cuda.empty_cache()
    say("\nevery batched call gave the single calls' bytes: %s" % ok)
    m.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
