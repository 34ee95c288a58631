"""Cost of revo_map_tsdf_shift / revo_map_tsdf_refill (api.VoxelMap.shift_into / refill_into; include/revo_hip.h) on one
GPU, written to profiles/map_follow_rates.txt.

DESIGN 26's protocol and scene (profiles/map_tsdf_ray_rates.py): the carving scene's 320x240 depth views, 2 cm voxels, a box of 256^3
cells around the map's median voxel, 8 views (the scene's four, twice) fused with their colour images; 3 warm-up calls, then the
median of `--reps` calls with the range, a host clock around one call and the wait for the stream, everything in device memory.  All
rows run in one process, alternating: one call of every row per round, so that what the machine does meanwhile falls on all of them.

  yardstick                      a device-to-device copy of both volumes (dst.copy_(src))
  shift, leaving cells dropped   shift_into with delta = (16, 0, 0)
  shift with records             the same shift with the records
  shift with records, diagonal   delta = (16, 16, 16)
  refill                         a refill of the (16, 0, 0) shift's records into a cleared box
  fixed cost                     the copy and the dropping shift over a 16^3 box: what a call costs before it moves a byte

No time is fixed in advance: the move touches at most the copy's bytes, so the copy is what it is measured against.

    python profiles/map_follow_rates.py [--reps 10] [--size 256] [--commit TEXT] [--out profiles/map_follow_rates.txt]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_follow_rates.txt"))
    a = ap.parse_args()
    import torch
    from revo_amd import api, mapfile
    import map_carve_cases as cc
    lines = []

    def say(text=""):
        print(text)
        sys.stdout.flush()
        lines.append(text)

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
    src_t = torch.zeros(n + (2,), dtype=torch.int32, device="cuda")
    src_c = torch.zeros(n + (4,), dtype=torch.int32, device="cuda")
    m.fuse_into(src_t, coloured, lo, d_color=src_c)
    dst_t, dst_c = torch.empty_like(src_t), torch.empty_like(src_c)
    cells = e ** 3
    flat, diag = (16, 0, 0), (16, 16, 16)
    info = {}
    for name, d in (("flat", flat), ("diag", diag)):
        info[name] = m.shift_into(dst_t, src_t, lo, d, dst_c, src_c, count_only=True)
    cap = max(info["flat"][0], info["diag"][0], 1)
    d_rec = torch.zeros(32 * cap, dtype=torch.uint8, device="cuda")
    d_flat = torch.zeros(32 * max(info["flat"][0], 1), dtype=torch.uint8, device="cuda")
    n_flat = m.shift_into(dst_t, src_t, lo, flat, dst_c, src_c, d_records=d_flat)[0]
    m.sync()
    fill_t, fill_c = torch.zeros_like(src_t), torch.zeros_like(src_c)
    s16_t, s16_c = torch.zeros((16, 16, 16, 2), dtype=torch.int32, device="cuda"), torch.zeros((16, 16, 16, 4), dtype=torch.int32, device="cuda")
    d16_t, d16_c = torch.empty_like(s16_t), torch.empty_like(s16_c)
    res = {}

    def copy():
        dst_t.copy_(src_t)
        dst_c.copy_(src_c)
        torch.cuda.synchronize()

    def dropped():
        m.shift_into(dst_t, src_t, lo, flat, dst_c, src_c)
        m.sync()

    def records():
        res["flat"] = m.shift_into(dst_t, src_t, lo, flat, dst_c, src_c, d_records=d_rec)
        m.sync()

    def diagonal():
        res["diag"] = m.shift_into(dst_t, src_t, lo, diag, dst_c, src_c, d_records=d_rec)
        m.sync()

    def refill():
        fill_t.zero_()
        fill_c.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res["refill"] = m.refill_into(fill_t, lo, d_flat, n_flat, d_color=fill_c)
        m.sync()
        return (time.perf_counter() - t0) * 1e3  # the clearing is not the refill's

    def copy16():
        d16_t.copy_(s16_t)
        d16_c.copy_(s16_c)
        torch.cuda.synchronize()

    def dropped16():
        m.shift_into(d16_t, s16_t, lo, (1, 0, 0), d16_c, s16_c)
        m.sync()

    fixed = [("fixed cost: copy, 16^3 box", copy16), ("fixed cost: shift dropped, 16^3 box", dropped16)]
    rows = [("yardstick: copy of both volumes", copy), ("shift, leaving cells dropped", dropped), ("shift with records", records),
            ("shift with records, diagonal", diagonal), ("refill", refill)]
    ms = {name: [] for name, _ in rows + fixed}
    for r in range(3 + a.reps):
        for name, fn in rows + fixed:
            t0 = time.perf_counter()
            own = fn()
            t = (time.perf_counter() - t0) * 1e3 if own is None else own
            if r >= 3:
                ms[name].append(t)
    stat = {name: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for name, v in ms.items()}
    base = stat[rows[0][0]]
    vol_bytes = cells * (8 + 16)
    say("Moving the surface volumes with their box, one MI355X, source: %s" % a.commit)
    say("scene: 8 views of %dx%d fused with colour, voxels of %g m, a box of %d^3 cells (%d cells, %.1f MB in both volumes);"
        % (s.width, s.height, cc.VOXEL, e, cells, vol_bytes / 1e6))
    say("median (min .. max) of %d calls after 3 warm-up calls, the rows alternating in one process, a host clock around the call and its wait,"
        % a.reps)
    say("everything in device memory")
    say("")
    say("%-34s %10s %20s %8s   %s" % ("row", "ms", "min .. max", "x copy", "cells: staying, leaving, records; bytes read + written"))
    for name, _ in rows:
        t = stat[name]
        note = ""
        if name.startswith("yardstick"):
            note = "%d cells; %.1f MB + %.1f MB" % (cells, vol_bytes / 1e6, vol_bytes / 1e6)
        elif name == "refill":
            i = res["refill"]
            note = "%d records applied, %d outside; %.1f MB of records twice (check, apply) + %.1f MB of cells read twice, written once" % (
                i["applied"], i["outside"], 32 * n_flat / 1e6, 24 * i["applied"] / 1e6)
        else:
            i = info["diag" if "diagonal" in name else "flat"][1]
            nrec = i["records"]
            passes = 0 if "dropped" in name else 2
            note = "%d, %d, %d; %.1f MB + %.1f MB moved, %.1f MB of leaving cells read %s, %.1f MB of records" % (
                i["staying"], i["leaving"], nrec, 24 * i["staying"] / 1e6, vol_bytes / 1e6, 24 * i["leaving"] / 1e6,
                "once (count)" if not passes else "twice (count, emit)", 0.0 if not passes else 32 * nrec / 1e6)
        say("%-34s %10.3f %9.3f .. %7.3f %8.2f   %s" % ((name,) + t + (t[0] / base[0], note)))
    for name, _ in fixed:
        t = stat[name]
        say("%-34s %10.3f %9.3f .. %7.3f %8.2f   4096 cells" % ((name,) + t + (t[0] / base[0],)))
    say("")
    say("the copy's own spread: %.3f ms (min .. max); a shift row exceeds the copy by more than that where its median - the copy's median > %.3f ms"
        % (base[2] - base[1], base[2] - base[1]))
    for name in ("shift, leaving cells dropped", "shift with records", "shift with records, diagonal"):
        say("%-34s median - copy's median = %+.3f ms" % (name, stat[name][0] - base[0]))
    say("shift with records - shift dropped = %+.3f ms: the scan, the emit pass and the wait for the count between them"
        % (stat["shift with records"][0] - stat["shift, leaving cells dropped"][0]))
    fc_, fs_ = stat[fixed[0][0]][0], stat[fixed[1][0]][0]
    say("without the fixed cost: copy %.3f ms, shift dropped %.3f ms (%.2f x), shift with records %.3f ms (%.2f x)"
        % (base[0] - fc_, stat["shift, leaving cells dropped"][0] - fs_, (stat["shift, leaving cells dropped"][0] - fs_) / (base[0] - fc_),
           stat["shift with records"][0] - fs_, (stat["shift with records"][0] - fs_) / (base[0] - fc_)))
    ok = res["flat"][0] == info["flat"][0] == n_flat and res["diag"][0] == info["diag"][0] and res["refill"]["applied"] == n_flat
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    m.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
