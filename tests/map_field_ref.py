"""The distance field of revo_map_distance_field (include/revo_hip.h) by its definition: every cell of the box against
every solid voxel inside it, in int64 -- independent of revo_amd.mapfile's separable form.  Test infrastructure only."""
import numpy as np

NONE = 0xFFFFFFFF
INFO_KEYS = ("cells", "solid", "outside", "below", "max_d2")


def key_axes(keys):
    k = np.asarray(keys, np.uint64)
    ax = [((k >> np.uint64(s)) & np.uint64(0x1FFFFF)).astype(np.int64) - (1 << 20) for s in (42, 21, 0)]
    return np.stack(ax, -1).reshape(-1, 3)


def brute_force(records, lo, n, min_count=1, clamp=0, chunk=1 << 22):
    """-> (d2 uint32 [n0, n1, n2], info dict).  chunk: the cell x voxel pairs formed at a time."""
    lo, n = np.asarray(lo, np.int64), np.asarray(n, np.int64)
    mc = max(1, int(min_count))
    cnt = records["count"].astype(np.int64)
    s = key_axes(records["key"][cnt >= mc])
    inside = np.all((s >= lo) & (s < lo + n), 1) if len(s) else np.zeros(0, bool)
    cells = int(n[0] * n[1] * n[2])
    info = {"cells": cells, "solid": int(inside.sum()), "outside": int(len(s) - inside.sum()), "below": int((cnt < mc).sum()), "max_d2": 0}
    s = s[inside]
    if len(s) == 0:
        return np.full(tuple(n), NONE, np.uint32), info
    c = np.stack(np.meshgrid(*[np.arange(lo[i], lo[i] + n[i], dtype=np.int64) for i in range(3)], indexing="ij"), -1).reshape(-1, 3)
    out = np.empty(cells, np.int64)
    step = max(1, chunk // len(s))
    for i in range(0, cells, step):
        d = c[i:i + step, None, :] - s[None, :, :]
        out[i:i + step] = (d * d).sum(-1).min(1)
    if clamp:
        out = np.minimum(out, int(clamp))
    info["max_d2"] = int(out.max())
    return out.astype(np.uint32).reshape(tuple(n)), info
