"""The cases shared by the unfuse tests (test_map_unfuse_cpu.py, test_gpu_map_unfuse.py): every fuse case of
map_tsdf_cases -- the boxes 1x1x1, 3x5x7 and 9x7x5 with lo < 0, 3x3x{1,3,4,5,33} for the tails of the kernel's runs of four, 1, 2, 4,
8 and 64 views -- with a seeded colour image per view and a split of its views into kept and removed ones: the first view, the last
one, every second one, all of them, and for the 64 views 63 of them.  The refusal cases are hand-set volumes with the number of
cells that do not FIT written out.  Test infrastructure only."""
import functools
import zlib

import numpy as np

import map_seen_cases as sc
import map_surface_cases as su
import map_surface_ref as sf
import map_tsdf_cases as tc
import map_tsdf_ref as tr

F = np.float32
V = tc.V
CELL, COLOR = tr.CELL, sf.COLOR


def splits(nv):
    """name -> the indices of the removed views, without the splits that name the same views twice."""
    out, seen = {}, set()
    for name, idx in (("first", [0]), ("last", [nv - 1]), ("every second", list(range(0, nv, 2))), ("all", list(range(nv))),
                      ("63 of 64", list(range(1, nv)) if nv == 64 else None)):
        if idx is None or tuple(idx) in seen:
            continue
        seen.add(tuple(idx))
        out[name] = idx
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(lo, n, views, trunc, bgr, removed, kept): removed and kept are indices into views."""
    c = {}
    for name, base in tc.fuse_cases().items():
        bgr = su.images(base["views"], zlib.crc32(name.encode()))
        nv = len(base["views"])
        for sname, removed in splits(nv).items():
            kept = [i for i in range(nv) if i not in set(removed)]
            c["%s / %s" % (name, sname)] = dict(base, bgr=bgr, removed=removed, kept=kept)
    return c


def pick(c, idx, color=True):
    """(views, bgr) of the case's views with the indices idx."""
    return [c["views"][i] for i in idx], [c["bgr"][i] for i in idx] if color else None


@functools.lru_cache(maxsize=None)
def fused(name, which):
    """The per-cell specification's volumes (cells, colour cells) of the case's views `which` ("all" or "kept"), computed once;
    zeros when there is no such view."""
    c = cases()[name]
    idx = list(range(len(c["views"]))) if which == "all" else c["kept"]
    if not idx:
        return np.zeros(tuple(c["n"]), CELL), np.zeros(tuple(c["n"]), COLOR)
    views, bgr = pick(c, idx)
    r = sf.fuse_color(V, c["lo"], c["n"], views, bgr, c["trunc"])
    return r[0], r[3]


# ---------------------------------------------------------------------------------------------------------- the refusals --
PLANE_IMAGE = np.full((12, 16, 3), 200, np.uint8)  # every pixel B = G = R = 200


def _plane(color=True):
    """The plane's view (trunc = M) fused alone into the box (LO, N): every named cell has weight 1."""
    view = (tc.depth_plane(), tc.I4, tc.KC)
    r = sf.fuse_color(V, tc.LO, tc.N, [view], [PLANE_IMAGE], tc.M)
    return view, r[0].copy(), r[3].copy()


def refusals():
    """name -> dict(lo, n, trunc, views, bgr, cells, color, misfits): volumes from which `views` cannot be taken, and how many
    cells say so.  Every case is refused with and without its colour volume, unless it is `color_only` or `tsdf_only` (there the
    count is written out for the TSDF rule alone); `tsdf_fits=False`: a colour-only case that the TSDF rule alone refuses too."""
    out = {}
    # a view that was never fused: every cell it would update has too little weight (or none)
    c = tc.fuse_cases()["two views"]
    bgr = su.images(c["views"], 7)
    a = sf.fuse_color(V, c["lo"], c["n"], c["views"][:1], bgr[:1], c["trunc"])
    b = tr.fuse(V, c["lo"], c["n"], c["views"][1:], c["trunc"])
    hit = b[0]["weight"] > 0  # the cells the second view updates
    short = hit & (a[0]["weight"] == 0)
    # where the first view gave a weight too the cell still misfits unless what is left is a state a fuse can reach
    q = b[0]["sum"].astype(np.int64)
    left = a[0]["sum"].astype(np.int64) - q
    both = hit & (a[0]["weight"] == 1)
    bad_both = both & (left != 0)  # w' = 0 needs s' = 0
    out["never fused"] = dict(lo=c["lo"], n=c["n"], trunc=c["trunc"], views=c["views"][1:], bgr=bgr[1:], cells=a[0], color=a[3],
                              misfits=int(short.sum() + bad_both.sum()), tsdf_only=True)
    # with the colour volume: a cell where both views gave one update and the sums cancel still misfits when the colour cell
    # does not return to zero -- the first view's update was CONFIRMED and the second's FREE (a colour weight would be left above
    # the TSDF weight 0), the other way round (the colour weight would go below zero), or both CONFIRMED on pixels whose bytes differ
    bc = sf.fuse_color(V, c["lo"], c["n"], c["views"][1:], bgr[1:], c["trunc"])[3]  # what the second view alone gives the colour cells
    left = {k: a[3][k].astype(np.int64) - bc[k].astype(np.int64) for k in ("sum_b", "sum_g", "sum_r", "weight")}
    colour_bad = both & ~bad_both & np.any([left[k] != 0 for k in left], axis=0)
    out["never fused, with colour"] = dict(lo=c["lo"], n=c["n"], trunc=c["trunc"], views=c["views"][1:], bgr=bgr[1:], cells=a[0], color=a[3],
                                           misfits=int(short.sum() + bad_both.sum() + colour_bad.sum()), color_only=True, tsdf_fits=False)
    # the same view out of an empty volume: every cell it updates
    out["empty volume"] = dict(lo=c["lo"], n=c["n"], trunc=c["trunc"], views=c["views"][1:], bgr=bgr[1:], cells=np.zeros(tuple(c["n"]), CELL),
                               color=np.zeros(tuple(c["n"]), COLOR), misfits=int(hit.sum()))
    # a weight that has reached 2^20: its history cannot be inverted
    w = tc.wall()
    vol, col = su.nearly_full(w["n"])
    img = [su.wall_image((1, 2, 3))]
    full = sf.fuse_color(V, w["lo"], w["n"], w["views"], img, w["trunc"], tsdf=vol, color=col)
    assert np.all(full[0]["weight"] == tr.W_MAX)
    out["full weight"] = dict(lo=w["lo"], n=w["n"], trunc=w["trunc"], views=w["views"], bgr=img, cells=full[0], color=full[3], misfits=int(vol.size))
    # the plane's view, one hand-set cell each
    view, cells, color = _plane()
    conf, free = tc.plane_cell("confirmed"), tc.plane_cell("free")  # q = 0 and q = 1024
    assert tuple(cells[conf]) == (0, 1) and tuple(cells[free]) == (1024, 1) and tuple(color[conf]) == (200, 200, 200, 1) and color[free]["weight"] == 0
    base = dict(lo=tc.LO, n=tc.N, trunc=tc.M, views=[view], bgr=[PLANE_IMAGE])
    v = cells.copy()
    v[conf] = (1024, 1)  # the view leaves weight 0 and sum 1024: |s'| <= 1024 w' fails
    out["sum left in an emptied cell"] = dict(base, cells=v, color=color, misfits=1)
    k = color.copy()
    k[conf] = (0, 0, 0, 0)
    out["colour weight too small"] = dict(base, cells=cells, color=k, misfits=1, color_only=True)
    k = color.copy()
    k[conf] = (199, 200, 200, 1)
    out["colour sum too small"] = dict(base, cells=cells, color=k, misfits=1, color_only=True)
    k = color.copy()
    k[free] = (0, 0, 0, 1)  # a FREE update takes the TSDF weight to 0 and leaves the colour weight 1
    out["colour weight above the TSDF weight"] = dict(base, cells=cells, color=k, misfits=1, color_only=True)
    k = color.copy()
    k[conf] = (200, 200, 456, 2)  # one update left, with a red sum above 255
    v = cells.copy()
    v[conf] = (0, 2)
    out["colour sum above 255 per update"] = dict(base, cells=v, color=k, misfits=1, color_only=True)
    return out


assert sc.V == V
