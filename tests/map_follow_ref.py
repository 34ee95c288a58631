"""Per-cell restatement of the contracts of a box that follows the camera (include/revo_hip.h revo_map_tsdf_shift /
revo_map_tsdf_refill), bit for bit, as the loops the contracts describe, without revo_amd.mapfile, whose vectorised
tsdf_shift_records / tsdf_refill_records / SurfaceStore are checked against it.

  key      ((x + 2^20) << 42) | ((y + 2^20) << 21) | (z + 2^20) of the voxel index (x, y, z)
  shift    the destination cell c' of the box lo + delta holds the source cell c' + delta when that lies in the source box, else
           zeros; a source cell whose c - delta is no destination cell is LEAVING; a leaving cell that is not EMPTY gives a record;
           records in ascending key order
  EMPTY    sum, weight and (with a colour volume) the four colour words are all zero
  FITS     weight <= 2^20, |sum| <= 2^30, colour weight <= 2^20, each colour sum <= 255 * 2^20
  refill   keys strictly ascending; a record inside the box is added word by word; all or nothing
  sequence the surface a following run holds is, per voxel index, the sum over the views whose box at the time held that index of
           that view's own fuse (map_tsdf_ref / map_surface_ref)
Test infrastructure only."""
import numpy as np

import map_surface_ref as sf
import map_tsdf_ref as tr

CELL, COLOR = tr.CELL, sf.COLOR
RECORD = np.dtype([("key", "<u8"), ("sum", "<i4"), ("weight", "<u4"), ("sum_b", "<u4"), ("sum_g", "<u4"), ("sum_r", "<u4"), ("color_weight", "<u4")])
SHIFT_KEYS = ("cells", "staying", "leaving", "records", "dropped")
REFILL_KEYS = ("records", "applied", "outside")
W_MAX, SUM_MAX, COLOR_MAX = 1 << 20, 1 << 30, 255 << 20
INDEX_MIN, INDEX_MAX = -(1 << 20), (1 << 20) - 1
COLOR_WORDS = ("sum_b", "sum_g", "sum_r", "weight")


def key(x, y, z):
    return ((int(x) + (1 << 20)) << 42) | ((int(y) + (1 << 20)) << 21) | (int(z) + (1 << 20))


def key_index(k):
    k = int(k)
    return ((k >> 42) & 0x1FFFFF) - (1 << 20), ((k >> 21) & 0x1FFFFF) - (1 << 20), (k & 0x1FFFFF) - (1 << 20)


def check_box(lo, n):
    if any(not 1 <= int(x) <= 1024 for x in n):
        raise ValueError("a box has 1 .. 1024 cells per axis")
    if any(int(l) < INDEX_MIN or int(l) + int(x) - 1 > INDEX_MAX for l, x in zip(lo, n)):
        raise ValueError("the box leaves the index range")
    if int(n[0]) * int(n[1]) * int(n[2]) > 1 << 27:
        raise ValueError("more than 2^27 cells")


def cell_words(cells, color, c):
    """(sum, weight, sum_b, sum_g, sum_r, colour weight) of the cell c as Python integers; no colour volume: zeros."""
    t = cells[c]
    col = (0, 0, 0, 0) if color is None else tuple(int(color[c][k]) for k in COLOR_WORDS)
    return (int(t["sum"]), int(t["weight"])) + col


def empty(words):
    return all(w == 0 for w in words)


def fits(words):
    s, w, b, g, r, cw = words
    return w <= W_MAX and abs(s) <= SUM_MAX and cw <= W_MAX and max(b, g, r) <= COLOR_MAX


def shift(cells, color, lo, delta):
    """-> (cells2, color2, records RECORD in ascending key order, info dict of SHIFT_KEYS with dropped = 0)."""
    n = cells.shape
    d = [int(x) for x in delta]
    check_box(lo, n)
    check_box([int(l) + x for l, x in zip(lo, d)], n)
    out = np.zeros(n, CELL)
    cout = None if color is None else np.zeros(n, COLOR)
    staying = 0
    for c in np.ndindex(*n):  # destination cells
        s = (c[0] + d[0], c[1] + d[1], c[2] + d[2])
        if all(0 <= s[k] < n[k] for k in range(3)):
            out[c] = cells[s]
            if color is not None:
                cout[c] = color[s]
            staying += 1
    rec = []
    leaving = 0
    for c in np.ndindex(*n):  # source cells, in place order
        t = (c[0] - d[0], c[1] - d[1], c[2] - d[2])
        if all(0 <= t[k] < n[k] for k in range(3)):
            continue
        leaving += 1
        w = cell_words(cells, color, c)
        if not empty(w):
            rec.append((key(lo[0] + c[0], lo[1] + c[1], lo[2] + c[2]),) + w)
    rec.sort(key=lambda r: r[0])
    total = n[0] * n[1] * n[2]
    assert staying + leaving == total
    return out, cout, np.array(rec, RECORD).reshape(-1), {"cells": total, "staying": staying, "leaving": leaving, "records": len(rec), "dropped": 0}


def refill(cells, color, lo, records):
    """-> (cells2, color2, info dict of REFILL_KEYS); ValueError where the call is refused.  The inputs are not changed."""
    n = cells.shape
    check_box(lo, n)
    out = cells.copy()
    cout = None if color is None else color.copy()
    prev, applied = None, 0
    for r in records:
        k = int(r["key"])
        if k >> 63 or (prev is not None and k <= prev):
            raise ValueError("keys must be strictly ascending")
        prev = k
        rc = tuple(int(r[f]) for f in ("sum_b", "sum_g", "sum_r", "color_weight"))
        if color is None and any(rc):
            raise ValueError("colour words without a colour volume")
        x, y, z = key_index(k)
        c = (x - int(lo[0]), y - int(lo[1]), z - int(lo[2]))
        if not all(0 <= c[i] < n[i] for i in range(3)):
            continue
        w = cell_words(out, cout, c)
        new = (w[0] + int(r["sum"]), w[1] + int(r["weight"])) + tuple(a + b for a, b in zip(w[2:], rc))
        if not fits(new):
            raise ValueError("a cell would not FIT")
        out[c] = (new[0], new[1])
        if cout is not None:
            cout[c] = new[2:]
        applied += 1
    return out, cout, {"records": len(records), "applied": applied, "outside": len(records) - applied}


class Store:
    """key -> the six words of a cell that has left: a dict, summed on equal keys."""

    def __init__(self):
        self.cells = {}

    def add(self, records):
        new = dict(self.cells)
        for r in records:
            w = (int(r["sum"]), int(r["weight"]), int(r["sum_b"]), int(r["sum_g"]), int(r["sum_r"]), int(r["color_weight"]))
            k = int(r["key"])
            new[k] = tuple(a + b for a, b in zip(new.get(k, (0,) * 6), w))
            if k >> 63 or not fits(new[k]):
                raise ValueError("a cell of the store would not FIT")
        self.cells = new

    def _inside(self, k, lo, n):
        return all(0 <= a - int(l) < int(m) for a, l, m in zip(key_index(k), lo, n))

    def records(self, keys=None):
        keys = sorted(self.cells) if keys is None else sorted(keys)
        return np.array([(k,) + self.cells[k] for k in keys], RECORD).reshape(-1)

    def take(self, lo, n):
        keys = [k for k in self.cells if self._inside(k, lo, n)]
        out = self.records(keys)
        for k in keys:
            del self.cells[k]
        return out

    def bounds(self):
        if not self.cells:
            return None
        idx = np.array([key_index(k) for k in self.cells], np.int64)
        return idx.min(0), idx.max(0) - idx.min(0) + 1

    def volume(self, lo, n):
        cells, color = np.zeros(tuple(int(x) for x in n), CELL), np.zeros(tuple(int(x) for x in n), COLOR)
        for k, w in self.cells.items():
            if self._inside(k, lo, n):
                c = tuple(a - int(l) for a, l in zip(key_index(k), lo))
                cells[c] = w[:2]
                color[c] = w[2:]
        return cells, color


def follow_lo(T_w_c, n, voxel, ahead, step):
    """The policy, axis by axis in Python floats (float64) from the float32 pose and voxel edge."""
    import math
    T = np.asarray(T_w_c, np.float32).reshape(4, 4)
    out = []
    for i in range(3):
        p = float(T[i, 3]) + float(ahead) * float(T[i, 2])
        want = math.floor(p / float(np.float32(voxel))) - int(n[i]) // 2
        lo = int(step) * (want // int(step))
        out.append(min(max(lo, INDEX_MIN), INDEX_MAX + 1 - int(n[i])))
    return out


def sequence(voxel, n, views, bgr, boxes, trunc=None):
    """The sequence rule: views[i] (depth, T_w_c, intrinsics) with colour image bgr[i] was fused while the box was at boxes[i] (its
    lo) -> {voxel index: the six words}, the sum over the views of each view's own fuse over its own box, zeros left out."""
    total = {}
    for v, im, lo in zip(views, bgr, boxes):
        cells, _, _, col, _ = sf.fuse_color(voxel, lo, n, [v], [im], trunc)
        for c in np.ndindex(*cells.shape):
            w = cell_words(cells, col, c)
            if not empty(w):
                idx = (int(lo[0]) + c[0], int(lo[1]) + c[1], int(lo[2]) + c[2])
                total[idx] = tuple(a + b for a, b in zip(total.get(idx, (0,) * 6), w))
    return total


def sequence_volume(total, lo, n):
    """The sequence rule's cells inside the box (lo, n) as dense volumes."""
    cells, color = np.zeros(tuple(int(x) for x in n), CELL), np.zeros(tuple(int(x) for x in n), COLOR)
    for idx, w in total.items():
        c = tuple(a - int(l) for a, l in zip(idx, lo))
        if all(0 <= c[i] < int(n[i]) for i in range(3)):
            cells[c] = w[:2]
            color[c] = w[2:]
    return cells, color
