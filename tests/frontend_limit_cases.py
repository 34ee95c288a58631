"""The geometry the front end accepts, restated, and one case at every limit of it.  Test infrastructure: no GPU is touched here.

build_geom (revo_amd/csrc/revo_host.hip) accepts: 1..6 levels; width and height <= 2048; at most 2048 tiles of 32 x 32 pixels;
width a multiple of 4 * 2^(levels-1), height of 2^(levels-1); every level a multiple of 16 pixels; a histogram patch that fits
its level at least once and at most 128 times across.  The kernels of revo_pyramid.hip carry fixed limits sized to that domain.
`accepted` restates the rules in build_geom's order, the selectors below restate which path of which kernel a size takes, CASES
names one geometry on each side of every switch (tests/test_frontend_limits_cpu.py proves with the oracle that each case lands
where this table says; tests/test_gpu_frontend_limits.py runs them bit for bit), REFUSED one geometry one step outside each rule.

The table of limits (the `rows` of a case):
   1  height 1025..2048: 64 row groups of up to 32 rows in k_edt_cols, 64 chunks in k_compact_walk
   2  k_edt_cols with 32 row groups on the byte path (512 < h <= 1024, w % 32 != 0)
   3  both sides of the row-group switches: h = 512 / 513 and 1024 / 1025
   4  width 2048 (the LDS row of k_edt_rows) and both sides of EDT_ROW_PX = 1280 (edt_rows 1: a strided loop over the quads)
   5  2048 tiles exactly (s_tile[2048] of k_edge_prefix / k_tile_count)
   6  the smallest levels: 16 pixels, heights below NMS_ROWS, a pyrDown source of 2 rows, a 16 x 1 top level
   7  widths that are 4 mod 8, at level 0 and as the top of a pyramid
   8  HS_MAX_BANDS = 32: the clamp of the band height in build_geom, 32 bands in k_hyst_seam
   9  HS_MAX_PAIRS = 6144: the seam pass hands the level to k_hyst
  10  hist_w = 128 exactly; histogram tiles wider than three bitmap words (patches of 67 pixels and more)
  11  fill-in above 640 x 480 pixels: one launch per level, and a fill-in that changes something
  12  frames of a batch at minimal strides (the batch test of the GPU file, on the cases of rows 2, 3, 6, 7, 10 and 1, 4)
  13  the refusals themselves (REFUSED)
"""
import numpy as np

from revo_amd.settings import ImgPyramidSettings
from test_gpu_configs import band_geometry, khyst_limits, _noise_rows  # noqa: F401  (restatements kept in one place)
from test_gpu_parity import _edge_cases

REVO_MAX_WIDTH, REVO_MAX_HEIGHT, REVO_MAX_TILES, REVO_MAX_LEVELS = 2048, 2048, 2048, 6
NMS_ROWS, EDT_ROW_PX, HS_MAX_BANDS, HS_MAX_PAIRS, HYST_LDS_MAX = 6, 1280, 32, 6144, 158720

# the rules of build_geom, in its order, by the words of its own message
RULE_MAX_LVL = "pyr_max_lvl must be 0"
RULE_LEVELS = "1..6 pyramid levels supported"
RULE_SIZE = "image size must be within 2048 x 2048 and 2048 tiles of 32 x 32 pixels"
RULE_MULTIPLE = "width must be a multiple of 4*2^(levels-1) and height of 2^(levels-1)"
RULE_PIXELS = "every level must have a multiple of 16 pixels"
RULE_PATCH = "hist_patch out of range for this level size"
RULES = (RULE_MAX_LVL, RULE_LEVELS, RULE_SIZE, RULE_MULTIPLE, RULE_PIXELS, RULE_PATCH)


def level_sizes(w, h, levels):
    return [(w >> l, h >> l) for l in range(levels)]  # (int)((float)w * 2^-l), camerapyr.h:98-103


def accepted(w, h, levels, hist_patch=(), pyr_max_lvl=0):
    """None, or the rule of build_geom (revo_host.hip:44-126) that refuses the geometry, checked in its order."""
    if pyr_max_lvl != 0:
        return RULE_MAX_LVL
    if levels < 1 or levels > REVO_MAX_LEVELS:
        return RULE_LEVELS
    if w <= 0 or h <= 0 or w > REVO_MAX_WIDTH or h > REVO_MAX_HEIGHT or tiles(w, h) > REVO_MAX_TILES:
        return RULE_SIZE
    if w % (4 << (levels - 1)) or h % (1 << (levels - 1)):
        return RULE_MULTIPLE
    for l, (lw, lh) in enumerate(level_sizes(w, h, levels)):
        if (lw * lh) % 16:
            return RULE_PIXELS
        patch = hist_patch[l] if l < len(hist_patch) else 0
        if patch > 0 and (lw // patch < 1 or lh // patch < 1 or lw // patch > 128):
            return RULE_PATCH
    return None


# ---- which path a size takes, each from the code it names -------------------------------------------------------------------

def edt_col_path(w, h):
    """k_edt_cols (revo_pyramid.hip, EDT_COL_GROUPS): (row groups, how a thread gets its column's edge bits, rows per group)."""
    groups = 64 if h > 1024 else (32 if h > 512 else 16)
    ncols = 1024 // groups
    return groups, "transpose" if w % 32 == 0 and ncols % 32 == 0 else "bytes", (h + groups - 1) // groups


def chunks(h):
    return (h + 31) // 32  # nchunk of build_geom: the 32-row chunks of k_compact_walk (CW_MAXCHUNK = 64)


def tiles(w, h):
    return ((w + 31) // 32) * ((h + 31) // 32)  # the 32 x 32 tiles of k_tile_count / k_edge_prefix (s_tile[2048])


def fill_form(w, h):
    return "one block" if w * h <= 640 * 480 else "per level"  # launch_fill


def edt_rows(w):
    return max(1, EDT_ROW_PX // w)  # build_geom: whole rows per k_edt_rows workgroup


def hist_w(w, patch):
    return w // patch


def hyst_form(w, h, levels, env=None):
    """launch_hyst: "banded" (k_hyst_band / k_hyst_seam / k_hyst_out) when forced or when some level's bitmaps and tables do not
    fit the one workgroup of k_hyst, else "single"."""
    force = (env or {}).get("REVO_HYST_BANDED")
    if force:
        return "banded" if force != "0" else "single"
    ec = 0
    for lw, lh in level_sizes(w, h, levels):
        wpr = (lw + 31) // 32
        nw = lh * wpr
        ec = max(ec, ((lh + 2) * wpr + 2) * 4 + (nw + (nw + 2) // 2) * 4)
    return "single" if ec + 4096 <= HYST_LDS_MAX else "banded"


def band_rows_unclamped(w, h, patch, band_words=2400):
    """build_geom's band height before the clamp to HS_MAX_BANDS bands (revo_host.hip:105-109)."""
    wpr = (w + 31) // 32
    unit = patch if patch > 0 else 4
    while unit % 4:
        unit *= 2
    return min(max(unit, (band_words // wpr) // unit * unit), h)


def band_words_of(env):
    return int((env or {}).get("REVO_HYST_BAND_WORDS", 2400))


def weak_plane(ro, gray, lo, hi):
    """The weak pixels of a gray level as test_gpu_configs.weak_runs_per_row takes them: NMS candidates above lo, not above hi."""
    return (ro.canny(gray, lo, lo) > 0) & ~(ro.canny(gray, hi, hi) > 0)


def _word_runs(row):
    """ids of the word-local runs of a padded boolean row (a run ends at every 32-pixel word border), -1 off the runs."""
    prev = np.zeros_like(row)
    prev[1:] = row[:-1]
    prev[::32] = False
    return np.where(row, np.cumsum(row & ~prev) - 1, -1)


def seam_pairs(weak, rows):
    """What k_hyst_seam appends to s_pair: for every seam (last row of a band, first row of the next) and every word-local weak
    run of the row above, one entry per distinct word-local weak run of the row below that it touches 8-connectedly -- in its
    own word column (pixels x-1, x, x+1) and the neighbouring words' last / first pixel, which is the same neighbourhood."""
    h, w = weak.shape
    wpr = (w + 31) // 32
    P = np.zeros((h, wpr * 32 + 2), bool)  # one dead pixel on either side
    P[:, 1:w + 1] = weak
    total = 0
    for yb in range(rows, h, rows):
        a, b = P[yb - 1, 1:-1], P[yb, 1:-1]
        ia, ib = np.full(wpr * 32 + 2, -1), np.full(wpr * 32 + 2, -1)
        ia[1:-1], ib[1:-1] = _word_runs(a), _word_runs(b)
        pairs = set()
        for d in (0, 1, 2):  # the run below at x-1, x, x+1
            m = (ia[1:-1] >= 0) & (ib[d:d + wpr * 32] >= 0)
            pairs.update(zip(ia[1:-1][m].tolist(), ib[d:d + wpr * 32][m].tolist()))
        total += len(pairs)
    return total


# ---- images: the kinds the suite has ---------------------------------------------------------------------------------------

def smooth_image(w, h):
    """test_gpu_parity.test_unusual_sizes_bit_exact's: smooth random colour, depth between 0.05 and 5.5 m with 15 % holes."""
    import scipy.ndimage as ndi
    r = np.random.default_rng(w * 1000 + h)
    g = ndi.gaussian_filter(r.uniform(0, 255, (h, w, 3)), (2.0, 2.0, 0))
    bgr = np.clip((g - g.mean()) * 9 + 128, 0, 255).astype(np.uint8)
    depth = r.uniform(0.05, 5.5, (h, w)).astype(np.float32)
    depth[r.uniform(0, 1, (h, w)) < 0.15] = 0.0
    return bgr, depth


def _flat_depth(w, h):
    return np.full((h, w), 1.5, np.float32)


def row_ends_image(w, h):
    """The smooth image in the left half; in the right half flat gray with one bright dash in the FIRST row of some columns and
    one in the LAST row of others: those columns hold an edge only at one end, so every row group of k_edt_cols takes its
    nearest edge from the carries of all the groups above (below) it."""
    bgr, depth = smooth_image(w, h)
    x0 = w // 2
    bgr[:, x0:] = 90
    bgr[0, x0 + 2:x0 + 6] = 250
    bgr[h - 1, x0 + 9:x0 + 13] = 250
    return bgr, depth


def far_edge_image(w, h):
    """Flat gray with a bright square of side max(3, min(w, h) / 5) in the bottom-right corner (test_gpu_edt_rows_window's):
    the pixels at the other end search almost the whole row / column."""
    k = max(3, min(w, h) // 5)
    g = np.full((h, w), 60, np.uint8)
    g[max(0, h - 1 - k):max(1, h - 1), w - 1 - k:w - 1] = 255
    return np.repeat(g[..., None], 3, 2), _flat_depth(w, h)


def _edge_case(name, w, h):
    s = ImgPyramidSettings.scaled(w, h, 1)
    for n, bgr, depth in _edge_cases(s):
        if n == name:
            return bgr, depth
    raise KeyError(name)


def noise_image(w, h, rows=None, at=None, seed=3):
    """test_gpu_configs._noise_rows: 128 + N(0, 6) in the first `rows` rows (all of them by default), flat 128 below; with `at`
    (a band height) instead in the two rows on either side of every multiple of `at`, i.e. at the seams of bands of that height
    only -- the bands then stay inside their label space while every seam is as dense as in full noise."""
    g = _noise_rows(h if rows is None else rows, w=w, h=h, sigma=6.0, seed=seed)
    if at:
        keep = np.zeros(h, bool)
        for y in range(at, h, at):
            keep[y - 2:y + 2] = True
        g[~keep] = 128
    depth = _flat_depth(w, h)
    depth[::7, ::5] = 0.0
    return np.repeat(g[..., None], 3, 2), depth


def image_of(case):
    kind, w, h = case["image"], case["w"], case["h"]
    if kind == "smooth":
        return smooth_image(w, h)
    if kind == "row ends":
        return row_ends_image(w, h)
    if kind == "far edge":
        return far_edge_image(w, h)
    if kind in ("cross", "flat"):
        return _edge_case(kind, w, h)
    if kind == "noise":
        return noise_image(w, h)
    if kind == "seam noise":
        return noise_image(w, h, at=band_geometry(w, h, 0, band_words_of(case["env"]))[0])  # (no case has both noise and a patch)
    raise KeyError(kind)


def flat_image(w, h):
    return _edge_case("flat", w, h)


def settings_of(case):
    return ImgPyramidSettings.scaled(case["w"], case["h"], case["levels"], hist_patch=tuple(case["hist_patch"]) + (0,) * 6,
                                     canny_threshold1=case["canny"][0], canny_threshold2=case["canny"][1])


# ---- the cases --------------------------------------------------------------------------------------------------------------

FORCED_64 = {"REVO_HYST_BANDED": "1", "REVO_HYST_BAND_WORDS": "64"}
CASES = {}


def _case(w, h, levels, rows, image="smooth", hist_patch=(), canny=(150, 100), env=None, batch=True, why=""):
    name = "%dx%dx%d %s" % (w, h, levels, image) + (" bands of %d words" % band_words_of(env) if env else "")
    assert name not in CASES, name
    CASES[name] = dict(w=w, h=h, levels=levels, hist_patch=tuple(hist_patch), canny=canny, env=dict(env or {}), image=image,
                       rows=tuple(rows), batch=batch, why=why)


# `why`: the one thing only this case witnesses, or the sibling that covers its rows (the census test reads this column)
# row 6 first: the smallest levels run first on the GPU
_case(4, 4, 1, (6, 7, 12), "far edge", canny=(60, 20), why="16 pixels as 4 x 4, one quad per row")
_case(16, 1, 1, (6, 12), "far edge", canny=(60, 20), why="a single row: every NMS neighbour row is outside the image")
_case(8, 2, 1, (6, 12), "far edge", canny=(60, 20), why="16 pixels as 8 x 2")
_case(16, 2, 1, (6,), why="sibling: 8x2x1 (two rows), 32x2x2 (its level 0 is wider)")
_case(12, 4, 1, (6, 7), why="4 mod 8 below 16 wide: a 16-pixel store group wraps over two rows")
_case(20, 4, 1, (6, 7), why="sibling: 12x4x1; the store group wraps at another phase")
_case(16, 16, 3, (6, 7), why="a pyramid whose top is 4 x 4")
_case(32, 2, 2, (6,), why="pyrDown from a source of 2 rows to a 16 x 1 top level")
_case(64, 4, 3, (6,), why="pyrDown 4 -> 2 -> 1 rows: both one-row and two-row thread groups")
_case(128, 8, 4, (6,), why="sibling: 64x4x3; four levels down to 16 x 1")
_case(32, 32, 4, (6, 7), why="sibling: 16x16x3; the top 4 x 4 under three pyrDowns")
# row 7
_case(44, 12, 1, (7,), why="4 mod 8, two words per row, the second with 12 pixels")
_case(100, 76, 1, (7,), why="4 mod 8, several NMS row groups and chunks")
_case(72, 40, 2, (7,), why="a pyramid whose top level (36 x 20) is 4 mod 8")
# rows 2 and 3
_case(72, 520, 1, (2,), why="32 row groups, byte path, rpg 17")
_case(104, 1024, 1, (2, 3), why="32 row groups of 32 full rows on the byte path")
_case(32, 512, 1, (3,), "row ends", why="h = 512: 16 groups of 32 rows")
_case(32, 513, 1, (3,), "row ends", why="h = 513: 32 groups, rpg 17, the last groups empty")
_case(32, 1024, 1, (3,), "row ends", why="h = 1024: 32 groups of 32 rows, transpose path")
_case(32, 1025, 1, (1, 3), "row ends", why="h = 1025: 64 groups, rpg 17")
# row 1
_case(64, 2048, 1, (1,), "far edge", canny=(60, 20), why="64 chunks and 64 full row groups; a column search of ~2000 rows")
_case(16, 2047, 1, (1,), why="odd height, rpg 32 with a short last group, 64 chunks with a short last chunk")
# row 4
_case(2048, 16, 1, (4,), "far edge", canny=(60, 20), why="width 2048: a row search of ~2000 pixels through the whole LDS row")
_case(2048, 8, 1, (4,), why="sibling: 2048x16x1; smooth content at the full width")
_case(2044, 4, 1, (4, 7), why="the widest width that is 4 mod 8: 511 quads over 320 lanes")
_case(1284, 4, 1, (4, 7), why="first width above EDT_ROW_PX: edt_rows 1")
_case(1280, 4, 1, (4,), why="the other side: width EDT_ROW_PX, one quad per lane")
# row 5 (and row 9's overflow on the shipped settings)
_case(2048, 1024, 1, (5,), batch=False, why="2048 tiles exactly, every tile with points")
_case(2048, 1024, 1, (5, 9), "seam noise", canny=(60, 20), batch=False,
      why="shipped band height: more than HS_MAX_PAIRS seam contacts, the level goes to the last-resort k_hyst")
# rows 8 and 9
_case(640, 512, 1, (8, 9), "noise", canny=(60, 20), env=FORCED_64, batch=False, why="32 bands by the clamp, pairs below the limit")
_case(640, 512, 1, (8,), "seam noise", canny=(60, 20), env={"REVO_HYST_BANDED": "1"}, batch=False,
      why="the other side of the clamp: 120-row bands, no clamp")
_case(1280, 512, 1, (9,), "noise", canny=(60, 20), env=FORCED_64, batch=False, why="32 bands by the clamp, pairs above the limit")
_case(2048, 432, 1, (9,), "seam noise", canny=(60, 20), batch=False, why="shipped band height: pairs just below the limit")
# row 10
_case(512, 64, 2, (10,), "cross", hist_patch=(4, 2), why="hist_w 128 at both levels, fill-in changes level 1")
_case(640, 40, 2, (10,), "cross", hist_patch=(5, 5), why="hist_w 128 at level 0, 64 at level 1 (the other side)")
_case(640, 140, 1, (10,), hist_patch=(70,), why="a patch above 66: histogram tiles that span four bitmap words")
_case(640, 140, 1, (10,), hist_patch=(70,), env={"REVO_HYST_BANDED": "1"}, batch=False,
      why="the same tiles counted by k_hyst_out (one band of 140 rows)")
# row 11
_case(1280, 244, 2, (11,), "cross", hist_patch=(20, 10), batch=False, why="fill-in per level, one level to fill")
_case(1280, 248, 3, (11,), "cross", hist_patch=(20, 10, 5), batch=False, why="fill-in per level, level 2 reads the filled level 1")
_case(640, 480, 2, (11,), "cross", hist_patch=(20, 10), batch=False, why="the other side: 640 x 480 pixels, one block for all levels")

BATCH_CASES = [n for n, c in CASES.items() if c["batch"]]

# ---- one step outside every rule: (w, h, levels, hist_patch, pyr_max_lvl) -> the rule that refuses ---------------------------
REFUSED = {
    "width 2052": ((2052, 4, 1, (), 0), RULE_SIZE),
    "height 2049": ((4, 2049, 1, (), 0), RULE_SIZE),
    "2112 tiles": ((2048, 1056, 1, (), 0), RULE_SIZE),
    "width 6": ((6, 8, 1, (), 0), RULE_MULTIPLE),
    "width 8 for 2 levels with height 3": ((8, 3, 2, (), 0), RULE_MULTIPLE),
    "8 pixels": ((8, 1, 1, (), 0), RULE_PIXELS),
    "level 2 of 8 pixels": ((32, 2, 3, (), 0), RULE_MULTIPLE),
    "level 2 of 8 pixels, height a multiple": ((32, 4, 3, (), 0), RULE_PIXELS),
    "hist_w 160": ((640, 40, 1, (4,), 0), RULE_PATCH),
    "patch larger than the level": ((64, 16, 1, (20,), 0), RULE_PATCH),
    "7 levels": ((1280, 960, 7, (), 0), RULE_LEVELS),
    "pyr_max_lvl 1": ((640, 480, 2, (), 1), RULE_MAX_LVL),
}


def refused_settings(geom):
    w, h, levels, patch, max_lvl = geom
    return ImgPyramidSettings(width=w, height=h, pyr_min_lvl=levels - 1 + max_lvl, pyr_max_lvl=max_lvl,
                              hist_patch=tuple(patch) + (0,) * 6)
