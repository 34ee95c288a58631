"""Cost of registering a cloud against the voxel map's distance field (api.VoxelMap.df_align_eval / df_align, api.localize;
revo_map_df_align_eval, revo_map_df_align in include/revo_hip.h) on one GPU, written to
profiles/map_df_align_rates.txt.

The scene is the dense 320x240 two-keyframe scene of tests/map_plane_cases.py at 2 cm; the field covers its bounds grown by 14
cells (a 0.24 m gate); the source is the same keyframes' map under D_4^-1 (about 5.6 voxels off).

  1. revo_map_df_align_eval with field, points and output on the device, 1 and 64 poses per call: a host clock around `--reps`
     enqueued calls that end in a wait for the stream, after 3 warm-up calls; evaluations (poses) and point evaluations a second;
  2. api.localize from the identity (bounds, field build, upload of the points, field stage, point-to-plane stage): wall time,
     median of `--reps` calls after one warm-up call, and the share of each stage measured on its own;
  3. the numpy restatement (mapfile.df_align_records) of one evaluation on this machine's CPU.

    python profiles/map_df_align_rates.py [--reps 10] [--commit TEXT] [--out profiles/map_df_align_rates.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
TWIST = np.array([0.02, -0.015, 0.012, 0.006, -0.005, 0.004])
MAX_DIST = 0.24


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_df_align_rates.txt"))
    a = ap.parse_args()
    import torch
    from revo_amd import api, mapfile, synth
    import map_plane_cases as mc
    lines = []

    def say(text=""):
        print(text)
        sys.stdout.flush()
        lines.append(text)

    from revo_amd.settings import ImgPyramidSettings
    s = ImgPyramidSettings.scaled(320, 240, 3, hist_patch=(10, 5, 0, 0, 0, 0))
    cam = api.CameraPyr(s)
    D = synth.se3_exp(4 * TWIST)
    dst, src = api.VoxelMap(cam, mc.VOXEL, dense=True), api.VoxelMap(cam, mc.VOXEL, dense=True)
    dst.merge_raw(mc.dense_scene_records(mc.VOXEL).astype(mapfile.RAW_DTYPE))
    src.merge_raw(mc.dense_scene_records(mc.VOXEL, np.linalg.inv(D)).astype(mapfile.RAW_DTYPE))
    pts = src.points()[0]
    lo, hi, _ = dst.bounds()
    lo, n = mapfile.padded_box(lo, hi, 14)
    d_d2 = torch.empty(tuple(int(x) for x in n), dtype=torch.int32, device="cuda")
    dst.distance_field_into(d_d2, lo, n)
    d_pts = torch.from_numpy(pts).cuda()
    say("Registration against the distance field, one MI355X, source: %s" % a.commit)
    say("scene map: %d voxels of %g m, field box %s = %d cells (%.1f MB); source: %d points about 5.6 voxels off"
        % (dst.info()["voxels"], dst.voxel, "x".join(str(int(x)) for x in n), int(np.prod(n)), 4 * float(np.prod(n)) / 1e6, len(pts)))

    say("\n1. revo_map_df_align_eval, field, points and records on the device (host clock over %d enqueued calls, then a wait)" % a.reps)
    say("%-8s %12s %16s %18s" % ("poses", "ms / call", "evaluations / s", "Mpoint-evals / s"))
    rng = np.random.default_rng(1)
    for nposes in (1, 64):
        poses = [synth.se3_exp(rng.uniform(-1, 1, 6) * 0.02).astype(np.float32) for _ in range(nposes)]
        d_out = torch.zeros(208 * nposes, dtype=torch.uint8, device="cuda")
        for r in range(3):
            dst.df_align_eval(d_d2, lo, d_pts, poses, MAX_DIST, (0, 0, 0), d_out=d_out)
        dst.sync()
        t0 = time.perf_counter()
        for r in range(a.reps):
            dst.df_align_eval(d_d2, lo, d_pts, poses, MAX_DIST, (0, 0, 0), d_out=d_out)
        dst.sync()
        dt = (time.perf_counter() - t0) / a.reps
        say("%-8d %12.3f %16.0f %18.1f" % (nposes, dt * 1e3, nposes / dt, nposes * len(pts) / dt / 1e6))

    say("\n2. api.localize(dst, src) from the identity, max_dist %.2f m: wall time, median of %d calls after one warm-up call" % (MAX_DIST, a.reps))
    wall = []
    for r in range(1 + a.reps):
        t0 = time.perf_counter()
        res = api.localize(dst, src, max_dist=MAX_DIST)
        wall.append(time.perf_counter() - t0)
    E = np.linalg.inv(D) @ res["T"].astype(np.float64)
    st = dict(res["stages"])
    say("%.1f ms; field stage %d iterations (status %d), plane stage %d iterations (status %d); ends %.3g m, %.3g rad from D_4"
        % (1e3 * float(np.median(wall[1:])), st["field"]["iterations"], st["field"]["status"], st["plane"]["iterations"], st["plane"]["status"],
           np.linalg.norm(E[:3, 3]), synth.rot_angle(np.eye(3), E[:3, :3])))
    t0 = time.perf_counter()
    dst.distance_field_into(d_d2, lo, n)
    t_field = time.perf_counter() - t0
    t0 = time.perf_counter()
    f = dst.df_align(d_d2, lo, d_pts, None, MAX_DIST)
    t_loop = time.perf_counter() - t0
    t0 = time.perf_counter()
    dst.align_plane(src, f["T"], max_dist=dst.voxel, centre=f["centre"])
    t_plane = time.perf_counter() - t0
    say("on their own: field build %.1f ms (%.3f ms on the device), field stage %.1f ms, plane stage %.1f ms"
        % (t_field * 1e3, dst.last_distance_field_ms(), t_loop * 1e3, t_plane * 1e3))

    say("\n3. the numpy restatement (mapfile.df_align_records), one evaluation, on the host CPU")
    d2 = d_d2.cpu().numpy().view(np.uint32)
    t0 = time.perf_counter()
    want = mapfile.df_align_records(d2, lo, n, dst.voxel, pts, np.eye(4, dtype=np.float32), MAX_DIST, (0, 0, 0))[0]
    dt = time.perf_counter() - t0
    got = dst.df_align_eval(d_d2, lo, d_pts, np.eye(4, dtype=np.float32), MAX_DIST, (0, 0, 0))
    say("%.1f ms (%d of %d points matched); the device's record holds the same bytes: %s" % (dt * 1e3, want["matched"], want["considered"], bytes(got) == want.tobytes()))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f_:
        f_.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
