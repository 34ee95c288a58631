"""Cost of revo_map_view_gain (api.VoxelMap.view_gain_into; include/revo_hip.h) on one GPU, beside the composition it
replaces, written to profiles/map_gain_rates.txt.

The carving scene's map (tests/map_carve_cases.py: two dense 320x240 keyframes, 2 cm) in boxes of 64^3, 128^3 and 256^3 cells
around the map's median voxel; the seen volume of each box is what the scene's first two depth views have looked at.  The
candidates are the scene's four poses under small random twists: 1, 64 and 1024 of them, seen through the context's 320x240
camera and through the same camera at a quarter of the resolution (80x60).  miss_depth 0, radius 1.  3 warm-up calls, then the
median of `--reps` calls, a host clock around one call and the wait for the stream, everything in device memory:

  1. view_gain_into: milliseconds per call and per pose, and the cell classifications per second.  The cells a pose classifies
     are the unknown cells of its cull range; they are counted here on the host, with the cull restated in numpy (a statistic,
     not a check), and given as a share of the box's cells beside the share the cull alone leaves;
  2. the composition for the first poses of the same list, one pose at a time: raycast_into, a device copy of the volume,
     observe_into(accumulate) on the copy, the count of changed unknown cells with torch -- milliseconds per pose;
  3. the ratio of the two per-pose times.

    python profiles/map_gain_rates.py [--reps 10] [--commit TEXT] [--out profiles/map_gain_rates.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def cull(T, k, size, radius, lo, n, voxel):
    """revo_gain_host.h's gain_cull in numpy -> (first cell, cells) per axis relative to the box, cells 0 when empty."""
    fx, fy, cx, cy, _, zmax = [float(x) for x in k]
    g = radius + 1.0
    xs = [(u - cx) / fx * zmax for u in (-g, size[0] - 1 + g)]
    ys = [(v - cy) / fy * zmax for v in (-g, size[1] - 1 + g)]
    R, o = T[:3, :3].astype(np.float64), T[:3, 3].astype(np.float64)
    tc = -(R.T @ o)
    scale = max([abs(zmax)] + [abs(a) for a in xs + ys]) + np.abs(o).sum() + np.abs(tc).sum()
    scale += sum(max(abs(lo[a]), abs(lo[a] + n[a])) * voxel for a in range(3))
    pad = scale * 2.0 ** -14
    pts = np.array([o] + [R @ np.array([x, y, zmax]) + o for x in xs for y in ys])
    first = np.maximum(np.floor((pts.min(0) - pad) / voxel) - 1, lo)
    last = np.minimum(np.ceil((pts.max(0) + pad) / voxel) + 1, np.asarray(lo) + np.asarray(n) - 1)
    if np.any(first > last):
        return np.zeros(3, np.int64), np.zeros(3, np.int64)
    return (first - lo).astype(np.int64), (last - first + 1).astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_gain_rates.txt"))
    a = ap.parse_args()
    import torch
    from revo_amd import api, mapfile, synth
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
        return float(np.median(ms))

    rec = cc.scene_records().astype(mapfile.RAW_DTYPE)
    s = cc.settings320()
    cam = api.CameraPyr(s)
    m = api.VoxelMap(cam, cc.VOXEL, dense=True)
    m.merge_raw(rec)
    centre = np.median(mapfile.key_axes(rec["key"]), 0).astype(np.int64)
    views = [(torch.from_numpy(np.ascontiguousarray(D)).cuda(), T, k) for D, T, k in cc.scene_views(False)]
    k320 = cc.intrinsics320()
    k80 = (k320[0] / 4, k320[1] / 4, (k320[2] + 0.5) / 4 - 0.5, (k320[3] + 0.5) / 4 - 0.5, k320[4], k320[5])
    cameras = [("80x60", k80, (80, 60)), ("320x240", k320, (320, 240))]
    rng = np.random.default_rng(25)
    base = cc.poses()
    poses = np.stack([(base[i % 4] @ synth.se3_exp(rng.uniform(-0.1, 0.1, 6))).astype(np.float32) for i in range(1024)])
    d_poses = torch.from_numpy(np.ascontiguousarray(poses.transpose(0, 2, 1))).cuda()
    d_info = torch.zeros(8, dtype=torch.int64, device="cuda")
    say("View gain of the voxel map, one MI355X, source: %s" % a.commit)
    say("scene map: %d voxels of %g m; the seen volume of a box is what the scene's first two 320x240 views have looked at;" % (len(rec), m.voxel))
    say("candidate poses: the scene's four poses under random twists; radius 1, miss_depth 0; median of %d calls after 3 warm-up calls" % a.reps)
    say("\n1. view_gain_into, everything in device memory (host clock around the call and its wait)")
    say("%-12s %-8s %6s %10s %9s %11s %12s %12s %13s %11s %11s" % ("box", "camera", "poses", "unknown", "call ms", "ms / pose", "in the cull", "classified", "Gclass / s", "free / pose", "hits / pose"))
    rows = {}
    for e in (64, 128, 256):
        lo, n = centre - e // 2, (e, e, e)
        d_seen = torch.zeros(n, dtype=torch.uint8, device="cuda")
        m.observe_into(d_seen, views[:2], lo)
        seen = d_seen.cpu().numpy()
        unknown = ~mapfile.seen_known(seen, 1, mapfile.solid_cells(rec, lo, np.asarray(n))[0])
        integral = np.zeros((e + 1,) * 3, np.int64)
        integral[1:, 1:, 1:] = unknown.cumsum(0).cumsum(1).cumsum(2)

        def box_sum(f, c):
            x0, y0, z0 = f
            x1, y1, z1 = f + c
            I = integral
            return int(I[x1, y1, z1] - I[x0, y1, z1] - I[x1, y0, z1] - I[x1, y1, z0] + I[x0, y0, z1] + I[x0, y1, z0] + I[x1, y0, z0] - I[x0, y0, z0])

        for cname, k, size in cameras:
            ranges = [cull(T, k, size, 1, lo, n, cc.VOXEL) for T in poses]
            for count in (1, 64, 1024):
                d_out = torch.zeros((count, 8), dtype=torch.int32, device="cuda")
                call = lambda: m.view_gain_into(d_out, d_seen, lo, d_poses[:count], camera=k[:4], size=size, zrange=k[4:], d_info=d_info)  # noqa: E731
                ms = clock(call)
                in_cull = sum(int(np.prod(c)) for _, c in ranges[:count])
                classified = sum(box_sum(f, c) for f, c in ranges[:count])
                out = d_out.cpu().numpy()
                rows[(e, cname, count)] = ms / count
                say("%-12s %-8s %6d %10d %9.3f %11.4f %11.1f%% %11.1f%% %13.3f %11.0f %11.0f"
                    % ("scene %d^3" % e, cname, count, int(d_info[2].item()), ms, ms / count, 100.0 * in_cull / (count * e ** 3),
                       100.0 * classified / (count * e ** 3), classified / ms / 1e6, out[:, 0].mean(), out[:, 3].mean()))

        say("\n2. the composition, one pose at a time: raycast_into, a copy of the volume, observe_into(accumulate), the count (scene %d^3)" % e)
        say("%-12s %-8s %6s %11s %20s" % ("box", "camera", "poses", "ms / pose", "same count as view_gain"))
        d_unknown = torch.from_numpy(unknown).cuda()
        for cname, k, size in cameras:
            d_depth = torch.zeros((size[1], size[0]), dtype=torch.float32, device="cuda")
            d_out = torch.zeros((8, 8), dtype=torch.int32, device="cuda")
            m.view_gain_into(d_out, d_seen, lo, d_poses[:8], camera=k[:4], size=size, zrange=k[4:])
            want = d_out.cpu().numpy()
            got = []

            def compose(T):
                m.raycast_into(d_depth, None, T, camera=tuple(k[:4]) + tuple(size), zrange=k[4:])
                copy = d_seen.clone()
                m.observe_into(copy, [(d_depth, T, k)], lo, accumulate=True)
                return int(((copy != d_seen) & d_unknown).sum().item())

            per = []
            for T in poses[:8]:
                got.append(compose(T))
                per.append(clock(lambda: compose(T), reps=max(3, a.reps // 2)))
            rows[(e, cname, "composition")] = float(np.median(per))
            say("%-12s %-8s %6d %11.3f %20s" % ("scene %d^3" % e, cname, 8, float(np.median(per)), got == (want[:, 0] + want[:, 1]).tolist()))
        say()

    say("3. per pose: the composition over view_gain_into at 1, 64 and 1024 poses a call")
    say("%-12s %-8s %14s %10s %10s %10s" % ("box", "camera", "composition ms", "x at 1", "x at 64", "x at 1024"))
    for e in (64, 128, 256):
        for cname, _, _ in cameras:
            c = rows[(e, cname, "composition")]
            say("%-12s %-8s %14.3f %10.1f %10.1f %10.1f" % ("scene %d^3" % e, cname, c, c / rows[(e, cname, 1)], c / rows[(e, cname, 64)], c / rows[(e, cname, 1024)]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
