"""The specification of planning through the map (revo_map_plan / revo_map_plan_paths) in pure Python, and a different
algorithm from both implementations: a heapq Dijkstra over the 26 moves where revo_amd.mapfile sweeps whole arrays and the
device relaxes tiles, and the downhill walk cell by cell.  Test infrastructure only."""
import heapq

import numpy as np

NONE = 0xFFFFFFFF
REACHED, UNREACHABLE, OUTSIDE, TRUNCATED = 0, 1, 2, 3
INFO_KEYS = ("cells", "free", "reachable", "max_cost", "seeds_used", "seeds_outside", "seeds_blocked")
# dx outermost, then dy, then dz, each -1, 0, 1, the cell itself skipped; the weight is 3, 4, 5 for 1, 2, 3 changed coordinates
MOVES = [(dx, dy, dz, 2 + (dx != 0) + (dy != 0) + (dz != 0)) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1) if dx or dy or dz]
assert len(MOVES) == 26 and sorted(set(m[3] for m in MOVES)) == [3, 4, 5]


def plan(d2, lo, seeds, r2):
    """(cost uint32 [n0, n1, n2], info dict): the contract of revo_map_plan, by Dijkstra.  seeds: rows (x, y, z, cost0)."""
    d2 = np.asarray(d2, np.uint32)
    n0, n1, n2 = d2.shape
    free = (d2 >= np.uint32(r2)).tolist()
    dist = {}
    heap = []
    used = outside = blocked = 0
    for x, y, z, c0 in (tuple(int(v) for v in s) for s in seeds):
        c = (x - int(lo[0]), y - int(lo[1]), z - int(lo[2]))
        if not (0 <= c[0] < n0 and 0 <= c[1] < n1 and 0 <= c[2] < n2):
            outside += 1
        elif not free[c[0]][c[1]][c[2]]:
            blocked += 1
        else:
            used += 1
            if c0 < dist.get(c, 1 << 62):
                dist[c] = c0
                heapq.heappush(heap, (c0, c))
    done = set()
    while heap:
        d, c = heapq.heappop(heap)
        if c in done:
            continue
        done.add(c)
        for dx, dy, dz, w in MOVES:
            u = (c[0] + dx, c[1] + dy, c[2] + dz)
            if 0 <= u[0] < n0 and 0 <= u[1] < n1 and 0 <= u[2] < n2 and free[u[0]][u[1]][u[2]] and d + w < dist.get(u, 1 << 62):
                dist[u] = d + w
                heapq.heappush(heap, (d + w, u))
    cost = np.full(d2.shape, NONE, np.uint32)
    for c, d in dist.items():
        cost[c] = d
    info = {"cells": int(d2.size), "free": int(np.sum(d2 >= np.uint32(r2))), "reachable": len(dist), "max_cost": max(dist.values()) if dist else 0,
            "seeds_used": used, "seeds_outside": outside, "seeds_blocked": blocked}
    return cost, info


def paths(cost, lo, starts, max_len):
    """A list of (cells [(x, y, z) absolute], status, the start's cost): the contract of revo_map_plan_paths."""
    n0, n1, n2 = cost.shape
    c = np.asarray(cost, np.uint32).tolist()
    out = []
    for s in starts:
        x, y, z = (int(v) - int(o) for v, o in zip(s, lo))
        if not (0 <= x < n0 and 0 <= y < n1 and 0 <= z < n2):
            out.append(([], OUTSIDE, NONE))
            continue
        v = c[x][y][z]
        if v == NONE:
            out.append(([], UNREACHABLE, NONE))
            continue
        v0, cells = v, []
        while True:
            cells.append((x + int(lo[0]), y + int(lo[1]), z + int(lo[2])))
            for dx, dy, dz, w in MOVES:
                ux, uy, uz = x + dx, y + dy, z + dz
                if 0 <= ux < n0 and 0 <= uy < n1 and 0 <= uz < n2 and c[ux][uy][uz] != NONE and c[ux][uy][uz] + w == v:
                    break
            else:
                out.append((cells, REACHED, v0))
                break
            if len(cells) == max_len:
                out.append((cells, TRUNCATED, v0))
                break
            x, y, z, v = ux, uy, uz, c[ux][uy][uz]
    return out


def tile_rounds(d2, lo, seeds, r2, tile=8):
    """The rounds a tile-wise relaxation needs in a CPU model of it: per round every marked tile is settled on its own cells
    against the halo as it stood before the round, and marks the neighbours whose halo holds a cell it lowered.  -> (cost as
    plan() gives it, rounds): the model of the device's schedule when every tile reads its halo before any neighbour writes."""
    d2 = np.asarray(d2, np.uint32)
    n = d2.shape
    INF = 1 << 30
    free = d2 >= np.uint32(r2)
    g = np.where(free, INF, -1).astype(np.int64)
    marked = set()
    for x, y, z, c0 in (tuple(int(v) for v in s) for s in seeds):
        c = (x - int(lo[0]), y - int(lo[1]), z - int(lo[2]))
        if all(0 <= c[k] < n[k] for k in range(3)) and free[c]:
            g[c] = min(g[c], c0)
            marked.add(tuple(v // tile for v in c))
    rounds = 0
    while marked:
        rounds += 1
        before = g.copy()
        nxt = set()
        for t in sorted(marked):
            a = [t[k] * tile for k in range(3)]
            b = [min(a[k] + tile, n[k]) for k in range(3)]
            ha = [max(a[k] - 1, 0) for k in range(3)]
            hb = [min(b[k] + 1, n[k]) for k in range(3)]
            blk = before[ha[0]:hb[0], ha[1]:hb[1], ha[2]:hb[2]].copy()
            own = tuple(slice(a[k] - ha[k], a[k] - ha[k] + b[k] - a[k]) for k in range(3))
            blk[own] = g[a[0]:b[0], a[1]:b[1], a[2]:b[2]]
            start = blk[own].copy()
            heap = [(int(blk[c]), c) for c in np.ndindex(*blk.shape) if 0 <= blk[c] < INF]
            heapq.heapify(heap)
            while heap:
                d, c = heapq.heappop(heap)
                if d > blk[c]:
                    continue
                for dx, dy, dz, w in MOVES:
                    u = (c[0] + dx, c[1] + dy, c[2] + dz)
                    if all(own[k].start <= u[k] < own[k].stop for k in range(3)) and blk[u] >= 0 and d + w < blk[u]:
                        blk[u] = d + w
                        heapq.heappush(heap, (d + w, u))
            g[a[0]:b[0], a[1]:b[1], a[2]:b[2]] = blk[own]
            for c in zip(*np.nonzero(blk[own] < start)):
                steps = [[0] + ([-1] if c[k] == 0 else []) + ([1] if c[k] == tile - 1 else []) for k in range(3)]
                for dx in steps[0]:
                    for dy in steps[1]:
                        for dz in steps[2]:
                            u = (t[0] + dx, t[1] + dy, t[2] + dz)
                            if u != t and all(0 <= u[k] * tile < n[k] for k in range(3)):
                                nxt.add(u)
        marked = nxt
    cost = np.where((g >= 0) & (g < INF), g, NONE).astype(np.uint32)
    return cost, rounds
