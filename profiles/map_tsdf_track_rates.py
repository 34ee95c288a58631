"""Cost of revo_map_tsdf_track_eval / revo_map_tsdf_track (api.VoxelMap.surface_track_eval / surface_track; include/revo_hip.h,
DESIGN 29) on one GPU, written to profiles/map_tsdf_track_rates.txt.

DESIGN 28's protocol and scene (profiles/map_tsdf_ray_rates.py): the carving scene's 320x240 depth views, 2 cm voxels, a box of 256^3
cells around the map's median voxel, 8 views (the scene's four, twice) fused with their colour images, trunc 8 cm; 3 warm-up
calls, then the median of `--reps` calls, a host clock around one call and the wait for the stream, everything in device memory.
surface_track_eval is timed on view 0's depth image at 1, 8 and 64 poses (the view's own pose and poses up to 2 voxels / 2 degrees
off), at stride 1 and stride 2; one full surface_track from a start 2 voxels and 2 degrees off.  The yardstick runs in the same
process: df_align_eval of the same number of points (the frame's back-projected pixels at that stride, holes included) against the
map's distance field over the same box, at the same poses.

    python profiles/map_tsdf_track_rates.py [--reps 10] [--size 256] [--commit TEXT] [--out profiles/map_tsdf_track_rates.txt]
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
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_tsdf_track_rates.txt"))
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
    m.merge_raw(rec)
    e = a.size
    lo, n = np.median(mapfile.key_axes(rec["key"]), 0).astype(np.int64) - e // 2, (e, e, e)
    frames = cc.scene_frames()[0]
    views = cc.scene_views(False)
    plain = [(torch.from_numpy(np.ascontiguousarray(D)).cuda(), T, k) for D, T, k in views] * 2
    coloured = [v + (torch.from_numpy(np.ascontiguousarray(frames[i % 4][0])).cuda(),) for i, v in enumerate(plain)]
    trunc = float(mapfile.tsdf_trunc(cc.VOXEL))
    d_tsdf = torch.zeros(n + (2,), dtype=torch.int32, device="cuda")
    d_color = torch.zeros(n + (4,), dtype=torch.int32, device="cuda")
    m.fuse_into(d_tsdf, coloured, lo, d_color=d_color)
    d_d2 = torch.zeros(n, dtype=torch.int32, device="cuda")
    m.distance_field_into(d_d2, lo, n)
    h, w = s.height, s.width
    k = cc.intrinsics320()
    truth = np.asarray(views[0][1], np.float32)
    centre = mapfile.tsdf_track_centre(lo, n, cc.VOXEL)
    rng = np.random.default_rng(29)
    poses = [truth]
    for _ in range(63):
        T = kc.about(truth, centre, int(rng.integers(3)), float(rng.uniform(-2, 2))).astype(np.float64)
        T[:3, 3] += rng.uniform(-2, 2, 3) * cc.VOXEL
        poses.append(T.astype(np.float32))
    poses = np.stack(poses)
    d_frame = plain[0][0]
    frame = (d_frame, None)
    d_out = torch.zeros(64 * 208, dtype=torch.uint8, device="cuda")
    say("Tracking a depth frame against the TSDF surface, one MI355X, source: %s" % a.commit)
    say("scene: 8 views of %dx%d, voxels of %g m, trunc %g m, a box of %d^3 cells; the frame is view 0's depth image; median (min .. max)"
        % (w, h, cc.VOXEL, trunc, e))
    say("of %d calls after 3 warm-up calls, a host clock around the call and its wait, everything in device memory" % a.reps)
    say("\n1. surface_track_eval, and df_align_eval of as many points against the map's distance field over the same box")
    say("%-28s %10s %20s %14s   %10s %20s %8s" % ("poses, stride", "ms", "min .. max", "Mpixel-poses/s", "df ms", "min .. max", "ratio"))
    ok = True
    D = views[0][0]
    for stride in (1, 2):
        ys, xs = np.meshgrid(np.arange(0, h, stride), np.arange(0, w, stride), indexing="ij")
        d = D[ys, xs].astype(np.float32)
        good = np.isfinite(d) & (d > k[4]) & (d < k[5])
        pts = np.stack([(xs - np.float32(k[2])) / np.float32(k[0]) * d, (ys - np.float32(k[3])) / np.float32(k[1]) * d, d], -1).astype(np.float32)
        pts[~good] = np.nan  # as many points as the stride visits pixels; a hole is a point that is skipped
        d_pts = torch.from_numpy(np.ascontiguousarray(pts.reshape(-1, 3))).cuda()
        for np_ in (1, 8, 64):
            def track():
                m.surface_track_eval(d_tsdf, lo, trunc, frame, poses[:np_], stride=stride, centre=centre, d_out=d_out)
                m.sync()

            def field():
                m.df_align_eval(d_d2, lo, d_pts, poses[:np_], trunc / 2, centre=centre, d_out=d_out)
                m.sync()
            t, f = clock(track), clock(field)
            say("%-28s %10.3f %9.3f .. %7.3f %14.1f   %10.3f %9.3f .. %7.3f %8.2f"
                % ("%d poses, stride %d" % (np_, stride), t[0], t[1], t[2], len(d_pts) * np_ / t[0] / 1e3, f[0], f[1], f[2], t[0] / f[0]))
        track()
        got = np.frombuffer(d_out.cpu().numpy().tobytes(), mapfile.TSDF_TRACK_DTYPE)
        say("stride %d at the frame's own pose: %d of %d pixels matched, %d skipped" % (stride, got["matched"][0], got["considered"][0], got["skipped"][0]))
        ok = ok and int(got["considered"][0]) == len(d_pts) and int(got["flags"].sum()) == 0
    say("\n2. one surface_track from a start 2 voxels and 2 degrees off")
    start = kc.about(truth, centre, 1, 2.0).astype(np.float64)
    start[0, 3] += 2 * cc.VOXEL
    start = start.astype(np.float32)
    res = {}

    def loop():
        res["r"] = m.surface_track(d_tsdf, lo, trunc, frame, start, centre=centre)
    t = clock(loop)
    r = res["r"]
    say("%-28s %10.3f %9.3f .. %7.3f   %d iterations, %s, %d pixels matched; from %.4f m %.4f rad to %.2e m %.2e rad off the view's pose"
        % (("surface_track",) + t + (r["iterations"], ("converged", "iteration limit", "lost")[r["status"]], r["info"].matched)
           + kc.pose_error(start, truth) + kc.pose_error(r["T"], truth)))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    m.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
