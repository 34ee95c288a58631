"""Witnesses for tests/frontend_limit_cases.py, from the oracle alone (no GPU): every case is a geometry build_geom accepts and
lands on the path of the kernel that its row of the table names; every switch of the table has a case on each side; the
refused geometries are refused by the rule the table says.  Only then does the bit-for-bit comparison of
tests/test_gpu_frontend_limits.py mean what it claims."""
import numpy as np
import pytest

from revo_amd.settings import PLANE_DT, PLANE_EDGES, PLANE_EDGES_ORIG, PLANE_GRAY

import frontend_limit_cases as fl
from test_gpu_configs import band_geometry, weak_runs_per_row

NO_EDGE = np.sqrt(np.float32(1e15))


@pytest.fixture(scope="module")
def ro():
    from oracle import ro as R
    return R


@pytest.fixture(scope="module")
def facts(ro):
    """name -> what the selectors and the oracle say about the case"""
    out = {}
    for name, c in fl.CASES.items():
        w, h, levels = c["w"], c["h"], c["levels"]
        s = fl.settings_of(c)
        bgr, depth = fl.image_of(c)
        op = ro.Pyramid(s, bgr, depth)
        op.makeKeyframe()
        groups, path, rpg = fl.edt_col_path(w, h)
        f = dict(c, name=name, top=fl.level_sizes(w, h, levels)[-1], groups=groups, path=path, rpg=rpg, chunks=fl.chunks(h),
                 tiles=fl.tiles(w, h), quads=(w // 4) * fl.edt_rows(w), fill=fl.fill_form(w, h),
                 hyst=fl.hyst_form(w, h, levels, c["env"]),
                 hist_w=[fl.hist_w(lw, p) for (lw, lh), p in zip(fl.level_sizes(w, h, levels), c["hist_patch"])],
                 edges0=int((op.read(PLANE_EDGES, 0) > 0).sum()), dt_max=float(op.read(PLANE_DT, 0).max()),
                 filled=[int((op.read(PLANE_EDGES, l) != op.read(PLANE_EDGES_ORIG, l)).sum()) for l in range(1, levels)])
        e0 = op.read(PLANE_EDGES, 0) > 0
        pad = np.zeros((fl.chunks(h) * 32, (w + 31) // 32 * 32), bool)
        pad[:h, :w] = e0
        f["tiles_with_edges"] = int(pad.reshape(fl.chunks(h), 32, -1, 32).any(axis=(1, 3)).sum())
        ys = [np.flatnonzero(e0[:, x]) for x in range(w)]  # columns whose only edges are next to the first / the last row
        f["top_only_cols"] = sum(1 for y in ys if len(y) and y.max() <= 2)
        f["bottom_only_cols"] = sum(1 for y in ys if len(y) and y.min() >= h - 3)
        f["wide_tile_edges"] = 0  # edge pixels in the fourth word of a level-0 histogram tile
        if c["hist_patch"]:
            p = c["hist_patch"][0]
            for tx in range(w // p):
                if (tx * p + p - 1) // 32 - (tx * p) // 32 > 2:
                    f["wide_tile_edges"] += int(e0[:h // p * p, ((tx * p) // 32 + 3) * 32:tx * p + p].sum())
        if f["hyst"] == "banded":
            assert levels == 1
            words, patch0 = fl.band_words_of(c["env"]), (c["hist_patch"] or (0,))[0]
            rows, capb = band_geometry(w, h, patch0, words)
            lo, hi = min(c["canny"]), max(c["canny"])
            gray = op.read(PLANE_GRAY, 0)
            runs = weak_runs_per_row(ro, gray, lo, hi)
            f.update(band_rows=rows, capb=capb, nbands=(h + rows - 1) // rows,
                     clamped=rows != fl.band_rows_unclamped(w, h, patch0, words),
                     band_runs=max(int(runs[r:r + rows].sum()) for r in range(0, h, rows)),
                     pairs=fl.seam_pairs(fl.weak_plane(ro, gray, lo, hi), rows))
        out[name] = f
    return out


def test_seam_pairs_on_a_hand_made_seam():
    """Two bands of 4 rows, 70 pixels wide (three words, the last with 6 pixels).  Row 3 / row 4:
    a run over pixels 2..5 above, runs 0..1, 3..3, 6..9 below: touches all three (x-1, x, x+1)  -> 3
    a run 30..33 above is two word-local runs (30..31 | 32..33); below one pixel at 31 and one at 32: each upper run touches
    both (own word, and the neighbour word's last / first pixel)                              -> 4
    a run at 40 above, a run at 42 below: no contact                                            -> 0
    a run 63..64 above (63 | 64), below 62 and 65: 63-62 and 64-65                              -> 2"""
    weak = np.zeros((8, 70), bool)
    weak[3, [2, 3, 4, 5, 30, 31, 32, 33, 40, 63, 64]] = True
    weak[4, [0, 1, 3, 6, 7, 8, 9, 31, 32, 42, 62, 65]] = True
    weak[0:3] = True  # rows away from the seam do not count
    weak[5:] = True
    assert fl.seam_pairs(weak, 4) == 3 + 4 + 0 + 2
    assert fl.seam_pairs(weak, 8) == 0  # one band: no seam


def test_every_case_is_accepted_and_has_an_edge(facts):
    for name, f in facts.items():
        assert fl.accepted(f["w"], f["h"], f["levels"], f["hist_patch"]) is None, name
        assert f["edges0"] > 0, name
        assert f["dt_max"] < NO_EDGE, name
        if f["image"] == "far edge" and max(f["w"], f["h"]) > 1024:  # the tall and the wide one: a pixel that searched more than half of the long side (test_gpu_edt_rows_window)
            assert f["dt_max"] > 0.5 * max(f["w"], f["h"]), (name, f["dt_max"])
        if f["image"] == "row ends":  # k_edt_cols reads the carries across every row group, downwards and upwards
            assert f["top_only_cols"] >= 2 and f["bottom_only_cols"] >= 2, (name, f["top_only_cols"], f["bottom_only_cols"])


def _banded(f, **kw):
    return f["hyst"] == "banded" and all(f[k] == v for k, v in kw.items())


# (row of the table, what must be witnessed, who witnesses it)
REQUIRED = [
    (1, "64 chunks and 64 full row groups", lambda f: f["chunks"] == 64 and (f["groups"], f["rpg"]) == (64, 32) and f["h"] % 32 == 0),
    (1, "rpg 32 with a short last group, a short last chunk", lambda f: (f["groups"], f["rpg"]) == (64, 32) and f["h"] % 32 != 0 and f["chunks"] == 64),
    (2, "32 groups on the byte path, rpg < 32", lambda f: (f["groups"], f["path"]) == (32, "bytes") and f["rpg"] < 32),
    (2, "32 groups on the byte path, rpg 32", lambda f: (f["groups"], f["path"], f["rpg"]) == (32, "bytes", 32)),
    (3, "h 512 with edges at the row ends", lambda f: f["h"] == 512 and f["image"] == "row ends" and f["groups"] == 16),
    (3, "h 513 with edges at the row ends", lambda f: f["h"] == 513 and f["image"] == "row ends" and f["groups"] == 32),
    (3, "h 1024 with edges at the row ends", lambda f: f["h"] == 1024 and f["image"] == "row ends" and (f["groups"], f["path"]) == (32, "transpose")),
    (3, "h 1025 with edges at the row ends", lambda f: f["h"] == 1025 and f["image"] == "row ends" and f["groups"] == 64),
    (4, "width 2048 with a search across the row", lambda f: f["w"] == 2048 and f["h"] < 32 and f["dt_max"] > 1500),
    (4, "width 2044", lambda f: f["w"] == 2044),
    (4, "321 quads for 320 lanes", lambda f: f["quads"] == 321),
    (4, "320 quads for 320 lanes at edt_rows 1", lambda f: f["quads"] == 320 and f["w"] == fl.EDT_ROW_PX),
    (5, "2048 tiles, an edge in every one", lambda f: f["tiles"] == 2048 and f["tiles_with_edges"] == 2048),
    (6, "a level 0 of 4 x 4", lambda f: (f["w"], f["h"]) == (4, 4)),
    (6, "a level 0 of 16 x 1", lambda f: (f["w"], f["h"]) == (16, 1)),
    (6, "a level 0 of 8 x 2", lambda f: (f["w"], f["h"]) == (8, 2)),
    (6, "width 12: a 16-pixel group over two rows", lambda f: f["w"] == 12 and f["h"] < fl.NMS_ROWS),
    (6, "three levels down to 4 x 4", lambda f: f["levels"] == 3 and f["top"] == (4, 4)),
    (6, "pyrDown from 2 rows to 16 x 1", lambda f: f["levels"] == 2 and f["h"] == 2 and f["top"] == (16, 1)),
    (6, "pyrDown from 4 rows to 2 to 1", lambda f: f["levels"] == 3 and f["h"] == 4 and f["top"] == (16, 1)),
    (7, "width 44", lambda f: f["w"] == 44 and f["w"] % 8 == 4),
    (7, "width 100 over several chunks", lambda f: f["w"] == 100 and f["chunks"] > 1),
    (7, "a top level that is 4 mod 8", lambda f: f["levels"] > 1 and f["top"][0] % 8 == 4 and f["top"][0] > 4),
    (8, "32 bands by the clamp, the seam pass within its pairs", lambda f: _banded(f, nbands=32, clamped=True) and f["pairs"] <= fl.HS_MAX_PAIRS),
    (8, "forced bands without the clamp", lambda f: _banded(f, clamped=False) and bool(f["env"]) and f["nbands"] > 1),
    (9, "more pairs than HS_MAX_PAIRS, forced bands", lambda f: _banded(f) and bool(f["env"]) and f["pairs"] > fl.HS_MAX_PAIRS),
    (9, "fewer pairs than HS_MAX_PAIRS on the shipped settings", lambda f: _banded(f) and not f["env"] and f["image"] == "seam noise" and f["pairs"] <= fl.HS_MAX_PAIRS),
    (9, "more pairs than HS_MAX_PAIRS on the shipped settings", lambda f: _banded(f) and not f["env"] and f["pairs"] > fl.HS_MAX_PAIRS),
    (10, "hist_w 128 at both levels", lambda f: f["hist_w"] == [128, 128] and f["filled"][0] > 0),
    (10, "hist_w 128 above hist_w 64", lambda f: f["hist_w"] == [128, 64]),
    (10, "histogram tiles over four bitmap words, edges in the fourth, k_hyst", lambda f: f["wide_tile_edges"] > 0 and f["hyst"] == "single"),
    (10, "histogram tiles over four bitmap words, edges in the fourth, k_hyst_out", lambda f: f["wide_tile_edges"] > 0 and _banded(f, nbands=1)),
    (11, "fill-in per level, two levels, level 1 changed", lambda f: f["fill"] == "per level" and f["levels"] == 2 and f["filled"][0] > 0),
    (11, "fill-in per level, levels 1 and 2 changed", lambda f: f["fill"] == "per level" and f["levels"] == 3 and min(f["filled"]) > 0),
    (11, "fill-in by one block at 640 x 480", lambda f: f["fill"] == "one block" and (f["w"], f["h"]) == (640, 480) and f["filled"][0] > 0),
]


def _witnesses(facts):
    return {label: [n for n, f in facts.items() if row in f["rows"] and pred(f)] for row, label, pred in REQUIRED}


def test_every_row_is_witnessed_on_each_side_of_its_switches(facts):
    wit = _witnesses(facts)
    for (row, label, pred) in REQUIRED:
        print("row %2d  %-58s %s" % (row, label, wit[label]))
        assert wit[label], "row %d: nothing witnesses '%s'" % (row, label)
    assert {r for r, _, _ in REQUIRED} == set(range(1, 12))
    assert {r for f in facts.values() for r in f["rows"]} == set(range(1, 13))  # 12: the batch test's cases; 13: REFUSED
    for name, f in facts.items():
        if f["hyst"] == "banded":
            # a band beyond its label space hands the level over before the seam pass counts anything
            print("%-34s %2d bands of %3d rows%s, runs per band <= %5d (capb %5d), seam pairs %5d"
                  % (name, f["nbands"], f["band_rows"], " (clamped)" if f["clamped"] else "", f["band_runs"], f["capb"], f["pairs"]))
            assert f["nbands"] <= fl.HS_MAX_BANDS, name
            assert f["band_runs"] <= f["capb"], name


def test_the_census_bites(facts):
    """Taking any one case away leaves a required witness without a case -- or the case names the sibling that covers its rows."""
    wit = _witnesses(facts)
    for name, f in facts.items():
        sole = [label for label, names in wit.items() if names == [name]]
        if f["why"].startswith("sibling: "):
            sib = [n for n in facts if n.startswith(f["why"][9:].split(";")[0].split(",")[0].split(" (")[0].strip() + " ")]
            assert sib, (name, f["why"])
            assert set(f["rows"]) <= set(facts[sib[0]]["rows"]) and not sole, (name, sib, sole)
        else:
            assert sole, "%s (%s) is the only witness of nothing" % (name, f["why"])


def test_batch_cases_are_the_small_ones():
    """Rows 2, 3, 6, 7 and 10 go through a batch of four frames as well, and the smaller cases of rows 1 and 4."""
    for name, c in fl.CASES.items():
        if set(c["rows"]) & {2, 3, 6, 7, 10} and not c["env"]:  # (a forced path of launch_hyst is a context's, not a batch's)
            assert c["batch"], name
        if c["batch"]:
            assert c["w"] * c["h"] <= 2048 * 64 and not c["env"], name
    assert {r for n in fl.BATCH_CASES for r in fl.CASES[n]["rows"]} >= {1, 2, 3, 4, 6, 7, 10, 12}


def test_refused_geometries_name_their_rule():
    seen = set()
    for what, (geom, rule) in fl.REFUSED.items():
        assert fl.accepted(*geom) == rule, (what, fl.accepted(*geom))
        seen.add(rule)
    assert seen == set(fl.RULES)
    # one step inside: the neighbours of the refused sizes are accepted
    for geom in ((2048, 4, 1), (4, 2048, 1), (2048, 1024, 1), (8, 8, 1), (8, 8, 2), (16, 1, 1), (64, 4, 3), (640, 40, 1, (5,)),
                 (64, 16, 1, (16,)), (1280, 960, 6)):
        assert fl.accepted(*geom) is None, geom
