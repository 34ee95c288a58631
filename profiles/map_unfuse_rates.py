"""Cost of revo_map_tsdf_unfuse (api.VoxelMap.unfuse_into; include/revo_hip.h) beside the fuse of the same views, and of
one api.SurfaceWindow.integrate beside one api.SurfaceVolume.integrate, on one GPU, written to profiles/map_unfuse_rates.txt.

The carving scene (tests/map_carve_cases.py: 320x240 depth views, 2 cm voxels) in a box of 256^3 cells around the map's median
voxel, as profiles/map_tsdf_rates.py has it; 8 views: the scene's four, twice, each with a seeded colour image.  Everything is in
device memory.  3 warm-up rounds, then the median of `--reps` rounds; a host clock around one call and the wait for the stream.

  1. a round is: fuse_into of the box from the 8 views (revo_map_tsdf_fuse[_color], not accumulating, so the volumes hold exactly
     these views), then unfuse_into of the same 8 views (all-zero volumes are left, which is checked), then unfuse_into of them
     once more: that one is refused by the check pass, so its time is the check pass and its wait alone.  The two calls alternate
     within a round, with and without the colour volume.
  2. a round is one integrate of a view and the wait: SurfaceVolume.integrate (one accumulating fuse), and SurfaceWindow.integrate
     at window 8 in its steady state (one fuse, then the unfuse of the oldest view), over the same views in the same order.

    python profiles/map_unfuse_rates.py [--reps 10] [--size 256] [--commit TEXT] [--out profiles/map_unfuse_rates.txt]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_unfuse_rates.txt"))
    a = ap.parse_args()
    import torch
    from revo_amd import api, mapfile
    import map_carve_cases as cc
    lines = []

    def say(text=""):
        print(text)
        sys.stdout.flush()
        lines.append(text)

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    rec = cc.scene_records().astype(mapfile.RAW_DTYPE)
    cam = api.CameraPyr(cc.settings320())
    m = api.VoxelMap(cam, cc.VOXEL, dense=True)
    m.merge_raw(rec)
    e = a.size
    lo, n = np.median(mapfile.key_axes(rec["key"]), 0).astype(np.int64) - e // 2, (e, e, e)
    rng = np.random.default_rng(32)
    views = [(torch.from_numpy(np.ascontiguousarray(D)).cuda(), T, k, torch.from_numpy(rng.integers(0, 256, D.shape + (3,), dtype=np.uint8)).cuda())
             for D, T, k in cc.scene_views(False)] * 2
    trunc = float(mapfile.tsdf_trunc(cc.VOXEL))
    cells = e ** 3
    d_tsdf = torch.zeros(n + (2,), dtype=torch.int32, device="cuda")
    d_color = torch.zeros(n + (4,), dtype=torch.int32, device="cuda")
    ok = True
    say("Views taken out of the TSDF surface again, one MI355X, source: %s" % a.commit)
    say("scene: %d views of 320x240 with colour images, voxels of %g m, trunc %g m, a box of %d^3 cells; median of %d rounds after 3 warm-up"
        % (len(views), cc.VOXEL, trunc, e, a.reps))
    say("rounds, a host clock around the call and its wait, everything in device memory")
    say("\n1. unfuse_into beside fuse_into of the same views (revo_map_tsdf_fuse[_color] is the parent commit's: this change does not touch it)")
    say("%-44s %10s %16s %10s" % ("call", "ms", "Gcell-views / s", "x fuse"))
    for color in (False, True):
        vs = views if color else [v[:3] for v in views]
        dc = d_color if color else None
        ms = {"fuse": [], "unfuse": [], "refused": []}
        info = None
        for r in range(3 + a.reps):
            t_f = timed(lambda: m.fuse_into(d_tsdf, vs, lo, d_color=dc))
            t_u = timed(lambda: m.unfuse_into(d_tsdf, vs, lo, d_color=dc))

            def again():
                try:
                    m.unfuse_into(d_tsdf, vs, lo, d_color=dc)
                except api.RevoError as err:
                    return err.info
                raise RuntimeError("an unfuse out of empty volumes was not refused")
            t0 = time.perf_counter()
            info = again()
            t_r = (time.perf_counter() - t0) * 1e3
            if r >= 3:
                ms["fuse"].append(t_f)
                ms["unfuse"].append(t_u)
                ms["refused"].append(t_r)
            ok = ok and not bool(d_tsdf.any().item()) and (not color or not bool(d_color.any().item()))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        tag = "with colour" if color else "TSDF alone"
        for k, name in (("fuse", "fuse_into"), ("unfuse", "unfuse_into (check + apply)"), ("refused", "unfuse_into refused (check)")):
            say("%-44s %10.3f %16.2f %10.2f" % ("%s, %s" % (name, tag), med[k], cells * len(vs) / med[k] / 1e6, med[k] / med["fuse"]))
        say("  spread of the unfuse over the rounds: %.3f .. %.3f ms; the refusal counted %d cells" % (min(ms["unfuse"]), max(ms["unfuse"]), info["misfits"]))
    say("all-zero volumes behind every fuse + unfuse: %s" % ok)
    say("\n2. one integrate of a view and the wait: SurfaceVolume beside SurfaceWindow at window 8 in its steady state (colour)")
    plain = api.SurfaceVolume(m, lo, n)
    window = api.SurfaceWindow(m, lo, n, window=8)
    for v in views:  # the window is full from here on
        window.integrate(v)
    m.sync()
    ms_p, ms_w = [], []
    for r in range(3 + a.reps):
        v = views[r % len(views)]
        t_p = timed(lambda: (plain.integrate(v), m.sync()))
        t_w = timed(lambda: (window.integrate(v), m.sync()))
        if r >= 3:
            ms_p.append(t_p)
            ms_w.append(t_w)
    mp, mw = float(np.median(ms_p)), float(np.median(ms_w))
    say("%-44s %10s %10s" % ("call", "ms", "x plain"))
    say("%-44s %10.3f %10.2f" % ("SurfaceVolume.integrate", mp, 1.0))
    say("%-44s %10.3f %10.2f" % ("SurfaceWindow.integrate", mw, mw / mp))
    say("  spread of the window's integrate: %.3f .. %.3f ms; it holds %d views" % (min(ms_w), max(ms_w), int(window.views)))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    m.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
