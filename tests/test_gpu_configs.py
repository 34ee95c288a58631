"""GPU parity across the reference's own configuration space and the kernels' data-dependent paths.

The rest of the GPU suite runs at one point of the settings space (TUM1: Canny 150/100, TUM1 intrinsics, depth 0.1-5.2 m,
USE_EDGE_HIST 1, nPercentage 0.3, USE_EDGE_FILTER 1, N_FRAMES_HIST_VOTING 3, CHECK_TRACKING_RESULTS 1, u16 depth at 5000).
Here the same bar -- every integer / per-element stage bit-exact with the oracle, the tracker within 1e-4 rad / 1e-4 m,
per-evaluation counts exact -- is held at:

* every shipped dataset configuration (tests/golden/reference_configs.json: TUM1, the Orbbec files, RealSense), end to end
  through the u16 entry points, single pair and batch, plus a dense-edge variant per Canny pair;
* Canny thresholds at their edges (contrasts t/4 - 1, t/4, t/4 + 1; swapped, equal, zero, huge thresholds);
* every code path of the single-workgroup hysteresis k_hyst, each case with a witness that asserts which path it takes;
* USE_EDGE_HIST 0, nPercentage, depths exactly at and next to DEPTH_MIN / DEPTH_MAX, every u16 depth value;
* USE_EDGE_FILTER 0, N_FRAMES_HIST_VOTING 0..4, CHECK_TRACKING_RESULTS 0, and sequential VO at the Orbbec configuration.
"""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from revo_amd import synth  # noqa: E402
from revo_amd.settings import (ImgPyramidSettings, OptimizerSettings, TrackerSettings, PLANE_DEPTH,  # noqa: E402
                               PLANE_EDGES, PLANE_EDGES_ORIG, PLANE_GRAY, TRACKER_STATE_NEW_KF)

from test_gpu_parity import (_edge_cases, assert_same, assert_tiled_list, compare_pyramid, rot_angle,  # noqa: E402,F401
                             ROT_TOL, TRANS_TOL)

HERE = os.path.dirname(os.path.abspath(__file__))
HIST = (20, 10, 5, 0, 0, 0)

# the cluster shape under which the single-pair launch and the batch partition the point lists identically
# (test_gpu_parity.py::test_batch_matches_single_and_full_size_properties): then the two agree bit for bit
SAME_PARTITION = {"REVO_TRACK_CLUSTER_ONE": "8", "REVO_TRACK_CLUSTER": "8", "REVO_TRACK_REDUNDANT_ONE": "400",
                  "REVO_TRACK_REDUNDANT_BATCH": "400"}


def _configs():
    """The distinct shipped dataset configurations, as (id naming every file that has these values, settings kwargs, scale)."""
    fix = json.load(open(os.path.join(HERE, "golden", "reference_configs.json")))
    out = {}
    for name in sorted(fix["datasets"]):
        v = fix["datasets"][name]
        kw = dict(width=v.get("width", 640), height=v.get("height", 480), fx=v["Camera.fx"], fy=v["Camera.fy"],
                  cx=v["Camera.cx"], cy=v["Camera.cy"], canny_threshold1=v["cannyThreshold1"],
                  canny_threshold2=v["cannyThreshold2"], depth_min=v["DEPTH_MIN"], depth_max=v["DEPTH_MAX"],
                  use_edge_hist=v["USE_EDGE_HIST"], n_percentage=v.get("nPercentage", 0.3))
        key = (tuple(sorted(kw.items())), v["DEPTH_SCALE_FACTOR"])
        out.setdefault(key, []).append(name)
    return [("+".join(names), dict(k[0]), k[1]) for k, names in out.items()]


CONFIGS = _configs()


def config_settings(kw, levels):
    return ImgPyramidSettings(pyr_min_lvl=levels - 1, hist_patch=HIST, **kw)  # (the reference has 3 patch sizes)


def to_u16(depth, scale):
    return np.clip(depth * scale, 0, 65535).astype(np.uint16)  # how the suite stores depth (iowrapperRGBD.cpp:326-327)


@pytest.fixture(scope="module")
def api():
    from revo_amd import api as A
    return A


@pytest.fixture(scope="module")
def ro():
    from oracle import ro as R
    return R


def eval_parity(tag, gt, ot, g_ref, g_cur, o_ref, o_cur, poses, levels):
    """test_residual_and_normal_equations_parity's bar: exact counts, err 1e-5 relative to the double-sum oracle, A / b 1e-4."""
    L = __import__("oracle.ro", fromlist=["lib"]).lib()
    L.ro_set_accum_double(1)
    try:
        for lvl in range(levels):
            for k, (R, T) in enumerate(poses):
                e_g, info_g, A_g, b_g = gt.mOptimizer.evalAt(g_ref, g_cur, R, T, lvl)
                e_o, info_o, A_o, b_o = ot.eval(o_ref, o_cur, R, T, lvl)
                assert info_g.good_pts_edges == info_o.good_pts_edges, (tag, lvl, k)
                assert info_g.bad_pts_edges == info_o.bad_pts_edges, (tag, lvl, k)
                assert info_o.good_pts_edges > 0, (tag, lvl, k)
                assert abs(e_g - e_o) <= 1e-5 * abs(e_o), (tag, lvl, k, e_g, e_o)
                scale = np.sqrt(np.outer(np.diag(A_o), np.diag(A_o)))
                assert np.all(np.abs(A_g - A_o) <= 1e-4 * scale), (tag, lvl, k)
                assert np.all(np.abs(b_g - b_o) <= 1e-4 * np.sqrt(np.diag(A_o)) * max(1.0, np.sqrt(e_o))), (tag, lvl, k)
    finally:
        L.ro_set_accum_double(0)


def three_poses(pair):
    gt_T = pair["T_ref_curr"]
    return [(np.eye(3), np.zeros(3)), (gt_T[:3, :3], gt_T[:3, 3]),
            (synth.se3_exp([0.02, -0.01, 0.03, 0.01, -0.02, 0.015])[:3, :3], np.array([0.02, -0.01, 0.03]))]


def same_record(rec, st, R, T, err, evals):
    return (np.array_equal(rec["R"], R) and np.array_equal(rec["T"], T) and rec["err"] == err and rec["status"] == st
            and np.array_equal(rec["evals"], evals))


# ---------------------------------------------------------------------------------------------------------------------
# 2. every shipped configuration, end to end


@pytest.mark.parametrize("levels", [3, 4])
@pytest.mark.parametrize("cfg", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_shipped_configuration_end_to_end(api, ro, monkeypatch, cfg, levels):
    """Synthetic pairs rendered with the configuration's intrinsics, depth as u16 at its DEPTH_SCALE_FACTOR, through the u16
    entry points: both pyramids (with a keyframe) bit-exact, trackFrames within tolerance of the oracle with the same status on
    4 pairs, and the batch's records equal to the single-pair results bit for bit."""
    import torch
    name, kw, scale = cfg
    for k, v in SAME_PARTITION.items():
        monkeypatch.setenv(k, v)
    s = config_settings(kw, levels)
    n = 4
    pairs = synth.make_pairs(range(700, 700 + n), s)
    cam = api.CameraPyr(s)
    trk = api.TrackerNew(TrackerSettings(), s, cam)
    ot = ro.Tracker(s)
    bgr = np.stack([p[k][0] for p in pairs for k in ("ref", "curr")])
    raw = np.stack([to_u16(p[k][1], scale) for p in pairs for k in ("ref", "curr")])
    single = []
    for i in range(n):
        g_ref = api.ImgPyramidRGBD(s, cam, bgr[2 * i], raw[2 * i], depth_scale_factor=scale)
        g_cur = api.ImgPyramidRGBD(s, cam, bgr[2 * i + 1], raw[2 * i + 1], depth_scale_factor=scale)
        g_ref.makeKeyframe()
        o_ref = ro.Pyramid(s, bgr[2 * i], ro.u16_to_depth(raw[2 * i], scale))
        o_cur = ro.Pyramid(s, bgr[2 * i + 1], ro.u16_to_depth(raw[2 * i + 1], scale))
        o_ref.makeKeyframe()
        if i == 0:
            compare_pyramid("cfg_%s_%d_ref" % (name, levels), g_ref, o_ref, s, True)
            compare_pyramid("cfg_%s_%d_cur" % (name, levels), g_cur, o_cur, s, False)
        st, R, T, err = trk.trackFrames(np.eye(3), np.zeros(3), g_ref, g_cur)
        r_o = ot.trackFrames(o_ref, o_cur, np.eye(3), np.zeros(3))
        dr, dt = rot_angle(R, r_o["R"]), float(np.linalg.norm(T - r_o["T"]))
        assert dr < ROT_TOL and dt < TRANS_TOL and st == r_o["status"], (name, levels, i, dr, dt, st, r_o["status"])
        single.append((st, R, T, err, trk.last_evals.copy()))
    bt = api.BatchTracker(cam, n)
    d_bgr, d_raw = torch.from_numpy(bgr).cuda(), torch.from_numpy(raw).cuda()
    d_res = torch.zeros(n * 96, dtype=torch.uint8, device="cuda")
    bt.build_u16(d_bgr.data_ptr(), d_raw.data_ptr(), scale)
    bt.track_only(d_res.data_ptr())
    bt.sync()
    res = api.results_from_buffer(d_res.cpu().numpy().tobytes(), n)
    for i in range(n):
        assert same_record(res[i], *single[i]), (name, levels, i)


@pytest.mark.parametrize("canny", sorted({(c[1]["canny_threshold1"], c[1]["canny_threshold2"]) for c in CONFIGS}),
                         ids=lambda c: "%d_%d" % c)
def test_dense_variant_per_canny_pair(api, ro, canny):
    """The same synthetic pair with N(0, 8) gray-level noise on the BGR: realistic edge density at the low thresholds.
    Bit-exact pyramids and per-evaluation parity at 3 poses per level; at 60/20 the level-0 list holds at least twice as many
    points as TUM1's clean pair on the same seed."""
    cfg = [c for c in CONFIGS if (c[1]["canny_threshold1"], c[1]["canny_threshold2"]) == canny][0]
    s = config_settings(cfg[1], 3)
    pair = synth.make_pair(711, s)
    base_n0 = ro.Pyramid(ImgPyramidSettings(), *synth.make_pair(711, ImgPyramidSettings())["curr"]).read(6, 0).shape[0]
    rng = np.random.default_rng(5)
    dense = dict(pair)
    for k in ("ref", "curr"):
        bgr, depth = pair[k]
        nz = rng.normal(0, 8, bgr.shape[:2])[..., None]
        dense[k] = (np.clip(np.rint(bgr + nz), 0, 255).astype(np.uint8), depth)
    cam = api.CameraPyr(s)
    gt = api.TrackerNew(TrackerSettings(), s, cam)
    ot = ro.Tracker(s)
    g_ref = api.ImgPyramidRGBD(s, cam, *dense["ref"])
    g_cur = api.ImgPyramidRGBD(s, cam, *dense["curr"])
    g_ref.makeKeyframe()
    o_ref, o_cur = ro.Pyramid(s, *dense["ref"]), ro.Pyramid(s, *dense["curr"])
    o_ref.makeKeyframe()
    compare_pyramid("dense%d_%d_ref" % canny, g_ref, o_ref, s, True)
    compare_pyramid("dense%d_%d_cur" % canny, g_cur, o_cur, s, False)
    counts = [g_cur.return3DEdges(l).shape[0] for l in range(3)]
    print("dense %d/%d: points per level %s (TUM1 clean pair, level 0: %d)" % (canny + (counts, base_n0)))
    if min(canny) == 20:
        assert counts[0] >= 2 * base_n0, (counts, base_n0)
    eval_parity("dense%d_%d" % canny, gt, ot, g_ref, g_cur, o_ref, o_cur, three_poses(pair), 3)


# ---------------------------------------------------------------------------------------------------------------------
# 3. Canny thresholds at their edges

def _step_image(w, h):
    """Bars of constant gray (B = G = R, so gray is the value exactly) on a flat 100: a bar of contrast c has two vertical step
    edges of Sobel magnitude 4c (|grad|^2 = 16 c^2, compared with floor(t^2) strictly).  Contrasts t/4 - 1, t/4, t/4 + 1 of
    every shipped threshold.  Per contrast: a bar that continues into a strong bar (weak touching strong) and a bar that
    touches nothing."""
    cs = sorted({int(t // 4) + d for t in (20, 50, 60, 80, 100, 150) for d in (-1, 0, 1)})
    img = np.full((h, w), 100, np.int32)
    for k, c in enumerate(cs):
        x0 = 6 + 17 * k
        img[10:h // 2, x0:x0 + 6] = 100 + c          # weak (at some thresholds) ...
        img[h // 2:h - 40, x0:x0 + 6] = 100 + 90     # ... continued by a strong bar
        # alone, over the full height: a bar's CORNER has |grad|^2 = 18 c^2 and would seed it (at 60/20 already for c = 15)
        img[:, x0 + 10:x0 + 14] = 100 + c
    assert 6 + 17 * len(cs) < w
    g = np.clip(img, 0, 255).astype(np.uint8)
    return np.repeat(g[..., None], 3, 2), cs


@pytest.mark.parametrize("thr", [(60, 20), (80, 50), (150, 100), (20, 60), (60, 60), (0, 0), (1500, 1500), (40000, 40000)],
                         ids=lambda t: "%d_%d" % t)
def test_canny_thresholds_at_their_edges(api, ro, thr):
    s = ImgPyramidSettings.scaled(320, 240, 3, hist_patch=(10, 5, 0, 0, 0, 0), canny_threshold1=thr[0], canny_threshold2=thr[1])
    bgr, cs = _step_image(320, 240)
    depth = np.full((240, 320), 1.5, np.float32)
    cam = api.CameraPyr(s)
    gp = api.ImgPyramidRGBD(s, cam, bgr, depth)
    op = ro.Pyramid(s, bgr, depth)
    gp.makeKeyframe()
    op.makeKeyframe()
    compare_pyramid("canny%d_%d" % thr, gp, op, s, True)
    e0 = gp.returnEdges(0)
    if min(thr) >= 1500:  # above the largest Sobel magnitude (4 * 255 * sqrt(2)); 40000 is clamped to 32767 before squaring
        assert not e0.any()
    if thr == (60, 20):
        # a step of contrast 15 gives |grad|^2 = 3600 = 60^2: not strong; contrast 16 is.  The lone bars: 15 -> no edge, 16 -> edge
        x15, x16 = [6 + 17 * cs.index(c) + 10 for c in (15, 16)]
        assert not e0[:, x15 - 2:x15 + 6].any() and e0[:, x16 - 2:x16 + 6].any()
    if thr in ((60, 20), (20, 60)):
        other = ImgPyramidSettings.scaled(320, 240, 3, hist_patch=(10, 5, 0, 0, 0, 0), canny_threshold1=thr[1],
                                          canny_threshold2=thr[0])
        cam2 = api.CameraPyr(other)
        g2 = api.ImgPyramidRGBD(other, cam2, bgr, depth)
        for lvl in range(3):
            assert_same("canny_swapped%d" % lvl, g2.returnEdges(lvl), gp.returnEdges(lvl))


@pytest.mark.parametrize("mode", ["default", "banded600", "banded2400"])
@pytest.mark.parametrize("size", [(320, 240), (640, 480)], ids=["320", "640"])
@pytest.mark.parametrize("canny", [(60, 20), (80, 50)], ids=["60_20", "80_50"])
def test_edge_cases_at_the_shipped_low_thresholds(api, ro, monkeypatch, canny, size, mode):
    w, h = size
    if mode != "default":
        monkeypatch.setenv("REVO_HYST_BANDED", "1")
        monkeypatch.setenv("REVO_HYST_BAND_WORDS", mode[6:])
    s = ImgPyramidSettings.scaled(w, h, 3, hist_patch=HIST if w == 640 else (10, 5, 0, 0, 0, 0),
                                  canny_threshold1=canny[0], canny_threshold2=canny[1])
    cam = api.CameraPyr(s)
    for name, bgr, depth in _edge_cases(s):
        gp = api.ImgPyramidRGBD(s, cam, bgr, depth)
        op = ro.Pyramid(s, bgr, depth)
        gp.makeKeyframe()
        op.makeKeyframe()
        compare_pyramid("lowthr%d_%d_%s_%dx%d_%s" % (canny + (mode, w, h, name)), gp, op, s, mode == "default")


# ---------------------------------------------------------------------------------------------------------------------
# 4. dense-edge hysteresis: every path of k_hyst, each case with a witness
#
# Limits of k_hyst<true> (revo_pyramid.hip, "union-find over the runs of weak pixels") for a level of w x h pixels:
#   wpr = ceil(w / 32) words per row, nwords = h * wpr, e_words = (h + 2) * wpr + 2 (edge bitmap with a zero row above and
#   below and a pad word at each end); the dynamic LDS holds REVO_HYST_LDS_MAX / 4 = 39680 words, of which the candidate
#   bitmap (nwords) and the 16-bit run-id bases (nwords + 2) / 2 are taken, leaving table_words for the union-find:
#   cap_keep = (table_words - e_words) / 2   runs whose parent + record tables end below the edge bitmap
#   cap      = min(table_words / 2, table_words - e_words)   runs one union-find can label (tables overlap the bitmap)
#   more runs than cap (and < 65536): the level is cut into bands of rows that fit cap, swept again while a band promotes in
#   its first row; >= 65536 runs overflow the 16-bit ids: the flood fill with the candidate bitmap in LDS.
# At 640 x 480 level 0 this is cap_keep 7818, cap 12639.
# The banded path (REVO_HYST_BANDED=1) labels at most band_capb runs per band (same file, band_capb(): a 64 KB band
# workgroup of HB_LDS_WORDS = 16384 words); a band beyond it sets need_full and k_hyst takes the whole (level, frame).

HYST_LDS_WORDS = 158720 // 4
HB_LDS_WORDS = 16384


def khyst_limits(w, h):
    wpr = (w + 31) // 32
    nwords = h * wpr
    e_words = (h + 2) * wpr + 2
    table_words = HYST_LDS_WORDS - (nwords + (nwords + 2) // 2)
    return (table_words - e_words) // 2, min(table_words // 2, table_words - e_words)


def band_geometry(w, h, patch, band_words=2400):
    """revo_host.hip build_geom (band rows: a multiple of the histogram patch and of 4) and band_capb()."""
    wpr = (w + 31) // 32
    unit = patch if patch > 0 else 4
    while unit % 4:
        unit *= 2
    rows = max(unit, (band_words // wpr) // unit * unit)
    rows = min(rows, h)
    if (h + rows - 1) // rows > 32:
        rows = ((h + 31) // 32 + unit - 1) // unit * unit
    nbands = (h + rows - 1) // rows
    nwb = rows * wpr
    table_words = HB_LDS_WORDS - (nwb + (nwb + 2) // 2)
    e_words = (rows + 2) * wpr + 2
    cap = min(table_words // 2, table_words - e_words, 65535)
    h_last = h - (nbands - 1) * rows
    cap = min(cap, ((h_last * w - 4 - 2 * wpr) // 8) * 5)
    return rows, max(cap, 0) & ~31


def weak_runs_per_row(ro, gray, lo, hi):
    """Horizontal runs of WEAK pixels (NMS candidates above lo, not above hi) inside each 32-pixel word, counted per row."""
    weak = (ro.canny(gray, lo, lo) > 0) & ~(ro.canny(gray, hi, hi) > 0)
    h, w = weak.shape
    wpr = (w + 31) // 32
    P = np.zeros((h, wpr * 32), bool)
    P[:, :w] = weak
    P = P.reshape(h, wpr, 32)
    prev = np.zeros_like(P)
    prev[:, :, 1:] = P[:, :, :-1]
    return (P & ~prev).sum(axis=(1, 2))


def khyst_row(runs, w, h):
    cap_keep, cap = khyst_limits(w, h)
    return "keep" if runs <= cap_keep else "overlap" if runs <= cap else "bands" if runs < 65536 else "floodfill"


def _noise_rows(rows, w=640, h=480, sigma=6.0, seed=3):
    """128 + N(0, sigma) in the first `rows` rows, flat 128 below: the weak-run count grows by ~147 per row at 640 wide."""
    rng = np.random.default_rng(seed)
    g = np.full((h, w), 128.0)
    g[:rows] = 128 + rng.normal(0, sigma, (h, w))[:rows]
    return np.clip(np.rint(g), 0, 255).astype(np.uint8)


def _serpentine(w=640, h=480, seed=4):
    """A weak serpentine bar (contrast 10 at 60/20: |grad|^2 <= 32 * 10^2 = 3200 < 60^2 everywhere, > 20^2 on its sides) that
    climbs from the bottom to the top of the level three times, seeded by a strong block at its bottom end only; noise on the
    right, separated by a flat margin, pushes the level past `cap`.  Each upward climb crosses every band seam upward, which
    only a re-sweep (or the fallback after 64 sweeps) promotes."""
    g = np.full((h, w), 128, np.int32)
    x = [30 + 50 * k for k in range(6)]
    for k, xk in enumerate(x):
        g[8:h - 8, xk:xk + 6] = 138
        if k + 1 < len(x):
            y = 8 if k % 2 == 0 else h - 14
            g[y:y + 6, xk:x[k + 1] + 6] = 138
    g[h - 20:h - 2, x[0] - 8:x[0] + 14] = 178  # the only strong seed, at the bottom end of the first climb
    rng = np.random.default_rng(seed)
    g[:, 340:] = np.rint(128 + rng.normal(0, 6, (h, w - 340)))
    return np.clip(g, 0, 255).astype(np.uint8), (slice(8, h - 8), slice(x[0], x[-1] + 6))


def _dense_cases():
    # crop heights found by bisection on the oracle's counts; the witnesses below assert where each lands
    for rows, want in ((52, "keep"), (53, "overlap"), (85, "overlap"), (86, "bands"), (240, "bands"), (446, "bands"),
                       (447, "floodfill"), (480, "floodfill")):
        yield "noise%d" % rows, _noise_rows(rows), want
    g, _ = _serpentine()
    yield "serpentine", g, "bands"


@pytest.fixture(scope="module")
def dense_hyst(ro):
    s = ImgPyramidSettings(canny_threshold1=60, canny_threshold2=20)
    depth = np.full((480, 640), 1.5, np.float32)
    depth[::7, ::5] = 0.0
    cases = []
    for name, g, want in _dense_cases():
        bgr = np.repeat(g[..., None], 3, 2)
        op = ro.Pyramid(s, bgr, depth)
        runs = [weak_runs_per_row(ro, op.read(PLANE_GRAY, l), 20, 60) for l in range(3)]
        cases.append((name, bgr, op, runs, want))
    return s, depth, cases


def test_dense_hysteresis_witnesses(ro, dense_hyst):
    """Every row of the k_hyst table is reached at level 0, one image on each side of each limit."""
    s, depth, cases = dense_hyst
    cap_keep, cap = khyst_limits(640, 480)
    assert (cap_keep, cap) == (7818, 12639)
    seen = set()
    for name, bgr, op, runs, want in cases:
        n0 = int(runs[0].sum())
        print("%-11s weak runs per level %s -> %s" % (name, [int(r.sum()) for r in runs], khyst_row(n0, 640, 480)))
        assert khyst_row(n0, 640, 480) == want, (name, n0)
        seen.add(want)
    assert seen == {"keep", "overlap", "bands", "floodfill"}
    near = sorted(int(c[3][0].sum()) for c in cases)
    for limit in (cap_keep, cap, 65535):  # within a few hundred runs on both sides of each limit
        assert any(limit - 300 <= r <= limit for r in near) and any(limit < r <= limit + 300 for r in near), limit
    # the serpentine: the oracle promotes the whole bar, which climbs across every band seam of the sweep
    name, bgr, op, runs, want = [c for c in cases if c[0] == "serpentine"][0]
    _, bar = _serpentine()
    n0 = int(runs[0].sum())
    nb = -(-n0 // cap)
    assert nb >= 3, n0
    e0 = op.read(PLANE_EDGES, 0)[bar]
    weak_bar = (ro.canny(op.read(PLANE_GRAY, 0), 20, 20) > 0)[bar]
    assert weak_bar.sum() > 3000 and np.array_equal(e0 > 0, weak_bar), "the oracle must promote every pixel of the bar"


def test_dense_hysteresis_single_frame(api, dense_hyst):
    s, depth, cases = dense_hyst
    cam = api.CameraPyr(s)
    for name, bgr, op, runs, want in cases:
        gp = api.ImgPyramidRGBD(s, cam, bgr, depth)
        compare_pyramid("hyst_single_" + name, gp, op, s, False)


def test_dense_hysteresis_batch(api, dense_hyst):
    """The same images as the frames of one BatchTracker of 8 (the default one-workgroup-per-(level, frame) k_hyst)."""
    import torch
    s, depth, cases = dense_hyst
    cam = api.CameraPyr(s)
    api.TrackerNew(TrackerSettings(), s, cam)
    assert 8 < len(cases) <= 16
    for chunk in (cases[:8], cases[8:] + cases[:16 - len(cases)]):
        bt = api.BatchTracker(cam, 4)
        d_bgr = torch.from_numpy(np.stack([c[1] for c in chunk])).cuda()
        d_dep = torch.from_numpy(np.stack([depth] * 8)).cuda()
        bt.build(d_bgr.data_ptr(), d_dep.data_ptr())
        bt.sync()
        for f, (name, bgr, op, runs, want) in enumerate(chunk):
            compare_pyramid("hyst_batch_" + name, bt.frame(f, s), op, s, False)


def test_dense_hysteresis_banded_handover(api, monkeypatch, dense_hyst):
    """REVO_HYST_BANDED=1: bands of 120 rows at level 0 whose runs exceed band_capb hand the (level, frame) to k_hyst
    (need_full), which then takes the path of the table above."""
    s, depth, cases = dense_hyst
    monkeypatch.setenv("REVO_HYST_BANDED", "1")
    rows, capb = band_geometry(640, 480, 20)
    assert (rows, capb) == (120, 6368)
    handed = 0
    for name, bgr, op, runs, want in cases:
        per_band = [int(runs[0][r:r + rows].sum()) for r in range(0, 480, rows)]
        handed += max(per_band) > capb
    print("bands of %d rows, %d runs each at most: %d of %d cases hand level 0 over" % (rows, capb, handed, len(cases)))
    assert handed >= len(cases) - 1
    cam = api.CameraPyr(s)
    for name, bgr, op, runs, want in cases:
        gp = api.ImgPyramidRGBD(s, cam, bgr, depth)
        compare_pyramid("hyst_banded_" + name, gp, op, s, False)


# ---------------------------------------------------------------------------------------------------------------------
# 5. pyramid flags and depth bounds

S320 = dict(hist_patch=(10, 5, 0, 0, 0, 0))


def test_use_edge_hist_off(api, ro):
    """USE_EDGE_HIST 0: no fill-in (edgesOrig == edges), pyramid and keyframe planes bit-exact, vote histograms equal."""
    s = ImgPyramidSettings.scaled(320, 240, 3, use_edge_hist=0, **S320)
    cam = api.CameraPyr(s)
    for name, bgr, depth in _edge_cases(s):
        gp = api.ImgPyramidRGBD(s, cam, bgr, depth)
        op = ro.Pyramid(s, bgr, depth)
        gp.makeKeyframe()
        op.makeKeyframe()
        compare_pyramid("nohist_" + name, gp, op, s, True)
        for lvl in range(3):
            assert_same("nohist_orig_" + name, gp._read(PLANE_EDGES_ORIG, lvl), gp._read(PLANE_EDGES, lvl))
    pair = synth.make_pair(31, s)
    gt = api.TrackerNew(TrackerSettings(), s, cam)
    ot = ro.Tracker(s)
    g_ref, g_cur = api.ImgPyramidRGBD(s, cam, *pair["ref"]), api.ImgPyramidRGBD(s, cam, *pair["curr"])
    o_ref, o_cur = ro.Pyramid(s, *pair["ref"]), ro.Pyramid(s, *pair["curr"])
    for k, P in enumerate((np.eye(4), synth.se3_exp([0.01, 0, 0.02, 0, 0.01, 0]), pair["T_ref_curr"])):
        gt.addOldPclAndPose(g_ref, 2, P, float(k))
        ot.addOldPclAndPose(o_ref, 2, P, float(k))
        st_g, h_g, o_g = gt.assessTrackingQuality(pair["T_ref_curr"], g_cur, return_hist=True)
        st_o, h_o, o_o = ot.assessTrackingQuality(pair["T_ref_curr"], o_cur)
        assert np.array_equal(h_g, h_o) and np.array_equal(o_g, o_o) and st_g == st_o, (k, h_g, h_o)


@pytest.mark.parametrize("pct", [0.0, 0.6, 1.0])
def test_n_percentage(api, ro, pct):
    s = ImgPyramidSettings.scaled(320, 240, 3, n_percentage=pct, **S320)
    cam = api.CameraPyr(s)
    changed = False
    for name, bgr, depth in _edge_cases(s):
        if name not in ("cross", "sparse"):
            continue
        gp = api.ImgPyramidRGBD(s, cam, bgr, depth)
        op = ro.Pyramid(s, bgr, depth)
        gp.makeKeyframe()
        op.makeKeyframe()
        compare_pyramid("npct%g_%s" % (pct, name), gp, op, s, True)
        changed = changed or not np.array_equal(op.read(PLANE_EDGES, 1), op.read(PLANE_EDGES_ORIG, 1))
    if pct == 0.6:
        assert changed, "fill-in must change level 1 at nPercentage 0.6"


def _boundary_depth(rng, h, w, dmin, dmax):
    f = np.float32
    vals = np.array([dmin, dmax, np.nextafter(f(dmin), f(0)), np.nextafter(f(dmin), f(10)), np.nextafter(f(dmax), f(0)),
                     np.nextafter(f(dmax), f(10)), 0.0, np.nan, np.inf, -np.inf, 1.0, 2.0], np.float32)
    return vals[rng.integers(0, len(vals), (h, w))], vals


def test_depth_range_boundaries(api, ro):
    """DEPTH_MIN 0.5 / DEPTH_MAX 3.0 with edge pixels holding exactly the bounds, their float neighbours, 0, NaN and +-inf
    (isPointOkDepth: isfinite && Z > min && Z < max, imgpyramidrgbd.h:170-173): lists, depth pyramid, coloured clouds and
    vote histograms bit for bit at every level."""
    s = ImgPyramidSettings.scaled(320, 240, 3, depth_min=0.5, depth_max=3.0, **S320)
    rng = np.random.default_rng(17)
    cam = api.CameraPyr(s)
    frames = []
    for name, bgr, _ in _edge_cases(s):
        if name in ("flat",):
            continue
        d, vals = _boundary_depth(rng, s.height, s.width, 0.5, 3.0)
        frames.append((name, bgr, d))
    # level 1 and 2 see the bounds too: 2x2 / 4x4 blocks of one value survive the subsample unchanged
    name, bgr, _ = frames[0]
    blocks = np.kron(vals[rng.integers(0, len(vals), (s.height // 4, s.width // 4))], np.ones((4, 4), np.float32))
    frames.append(("blocks", bgr, blocks.astype(np.float32)))
    gt = api.TrackerNew(TrackerSettings(), s, cam)
    ot = ro.Tracker(s)
    for name, bgr, d in frames:
        gp = api.ImgPyramidRGBD(s, cam, bgr, d)
        op = ro.Pyramid(s, bgr, d)
        gp.makeKeyframe()
        op.makeKeyframe()
        compare_pyramid("dbound_" + name, gp, op, s, True)
        for lvl in range(3):
            for dense in (False, True):
                assert_same("dbound_pcl_%s_%d_%d" % (name, lvl, dense), gp.generateColoredPcl(lvl, dense),
                            op.generateColoredPcl(lvl, dense))
        gt.addOldPclAndPose(gp, 2, np.eye(4), 0.0)
        ot.addOldPclAndPose(op, 2, np.eye(4), 0.0)
        st_g, h_g, o_g = gt.assessTrackingQuality(synth.se3_exp([0.01, 0, 0.01, 0, 0.01, 0]), gp, return_hist=True)
        st_o, h_o, o_o = ot.assessTrackingQuality(synth.se3_exp([0.01, 0, 0.01, 0, 0.01, 0]), op)
        assert np.array_equal(h_g, h_o) and np.array_equal(o_g, o_o) and st_g == st_o, (name, h_g, h_o)
        gt.clearUpPastLists()
        ot.clearUpPastLists()
    # the bounds themselves must have been on edge pixels, and been rejected
    gp = api.ImgPyramidRGBD(s, cam, frames[-1][1], frames[-1][2])
    z = gp.return3DEdges(0)[:, 2]
    assert len(z) and np.all((z > np.float32(0.5)) & (z < np.float32(3.0)))


# ---------------------------------------------------------------------------------------------------------------------
# 6. u16 depth conversion, exhaustively

@pytest.mark.parametrize("scale", [1000.0, 5000.0])
def test_every_u16_depth_value(api, ro, scale):
    import torch
    s = ImgPyramidSettings(canny_threshold1=60, canny_threshold2=20)
    n = 640 * 480
    raw = np.tile(np.arange(65536, dtype=np.uint16), n // 65536 + 1)[:n].reshape(480, 640)
    raw2 = np.ascontiguousarray(np.roll(raw, 12345))
    bgr = np.repeat(_noise_rows(480, sigma=10.0, seed=8)[..., None], 3, 2)
    cam = api.CameraPyr(s)
    api.TrackerNew(TrackerSettings(), s, cam)
    bt = api.BatchTracker(cam, 1)
    d_bgr = torch.from_numpy(np.stack([bgr, bgr])).cuda()
    d_raw = torch.from_numpy(np.stack([raw, raw2])).cuda()
    bt.build_u16(d_bgr.data_ptr(), d_raw.data_ptr(), scale)
    bt.sync()
    for f, r in enumerate((raw, raw2)):
        dep = ro.u16_to_depth(r, scale)
        op = ro.Pyramid(s, bgr, dep)
        gp = api.ImgPyramidRGBD(s, cam, bgr, r, depth_scale_factor=scale)
        assert_same("u16all_conv", gp.returnDepth(0), dep)
        compare_pyramid("u16all_%g_%d" % (scale, f), gp, op, s, False)
        view = bt.frame(f, s)
        for lvl in range(3):
            assert_same("u16all_batch_depth%d" % lvl, view.returnDepth(lvl), op.read(PLANE_DEPTH, lvl))
            assert_same("u16all_batch_pts%d" % lvl, view.return3DEdges(lvl), op.read(6, lvl))


# ---------------------------------------------------------------------------------------------------------------------
# 7. tracker and vote settings

def _filt0():
    ts = TrackerSettings()
    ts.optimizerSettings = OptimizerSettings(use_edge_filter=0)
    return ts


def test_edge_filter_off(api, ro, monkeypatch):
    """USE_EDGE_FILTER 0 (the filt arms of k_track's cost, retry and normal-equation paths): per-evaluation parity with exact
    counts, trackFrames parity on 8 pairs, batch records == single-pair records, one Pipeline step == the batch."""
    import torch
    for k, v in SAME_PARTITION.items():
        monkeypatch.setenv(k, v)
    s = ImgPyramidSettings.scaled(320, 240, 3, **S320)
    n = 8
    pairs = synth.make_pairs(range(720, 720 + n), s)
    ts = _filt0()
    cam = api.CameraPyr(s)
    gt = api.TrackerNew(ts, s, cam)
    ot = ro.Tracker(s, ts.optimizerSettings, ts)
    single = []
    for i, p in enumerate(pairs):
        g_ref, g_cur = api.ImgPyramidRGBD(s, cam, *p["ref"]), api.ImgPyramidRGBD(s, cam, *p["curr"])
        g_ref.makeKeyframe()
        o_ref, o_cur = ro.Pyramid(s, *p["ref"]), ro.Pyramid(s, *p["curr"])
        o_ref.makeKeyframe()
        if i == 0:
            # + a pose far enough off that residuals pass edge_distance_lvl (optimizer.cpp:108) and the filter matters
            far = synth.se3_exp([0.15, -0.1, 0.1, 0.08, -0.1, 0.06])
            poses = three_poses(p) + [(far[:3, :3], far[:3, 3])]
            eval_parity("filt0", gt, ot, g_ref, g_cur, o_ref, o_cur, poses, 3)
            ot1 = ro.Tracker(s, OptimizerSettings(), TrackerSettings())
            differs = 0
            for lvl in range(3):
                for R, T in poses:
                    i1, i0 = ot1.eval(o_ref, o_cur, R, T, lvl)[1], ot.eval(o_ref, o_cur, R, T, lvl)[1]
                    differs += (i1.good_pts_edges, i1.bad_pts_edges) != (i0.good_pts_edges, i0.bad_pts_edges)
            assert differs > 0, "USE_EDGE_FILTER 0 must change some count here"
        st, R, T, err = gt.trackFrames(np.eye(3), np.zeros(3), g_ref, g_cur)
        r_o = ot.trackFrames(o_ref, o_cur, np.eye(3), np.zeros(3))
        dr, dt = rot_angle(R, r_o["R"]), float(np.linalg.norm(T - r_o["T"]))
        assert dr < ROT_TOL and dt < TRANS_TOL and st == r_o["status"], (i, dr, dt)
        single.append((st, R, T, err, gt.last_evals.copy()))
    bgr = torch.from_numpy(np.stack([p[k][0] for p in pairs for k in ("ref", "curr")])).cuda()
    dep = torch.from_numpy(np.stack([p[k][1] for p in pairs for k in ("ref", "curr")])).cuda()
    bt = api.BatchTracker(cam, n)
    d_res = torch.zeros(n * 96, dtype=torch.uint8, device="cuda")
    bt.track(bgr.data_ptr(), dep.data_ptr(), d_res.data_ptr())
    bt.sync()
    raw = d_res.cpu().numpy().tobytes()
    res = api.results_from_buffer(raw, n)
    for i in range(n):
        assert same_record(res[i], *single[i]), i
    pipe = api.Pipeline(cam, n, depth=2)
    out = torch.zeros(n * 96, dtype=torch.uint8, device="cuda")
    pipe.submit(bgr.data_ptr(), dep.data_ptr(), out.data_ptr())
    pipe.drain()
    assert out.cpu().numpy().tobytes() == raw
    pipe.close()


# past clouds (alternately the reference and the current frame at these world poses) and the poses voted at
_FAR = synth.se3_exp([0.3, 0, 0, 0, 0.2, 0])
VOTE_POSES = [_FAR, synth.se3_exp([0.25, 0.1, 0, 0.1, 0, 0.1]), _FAR, np.eye(4), synth.se3_exp([0.01, 0, 0.02, 0, 0.01, 0])]
VOTE_QUERIES = [np.eye(4), _FAR, synth.se3_exp([0.05, 0.02, 0, 0, 0.05, 0])]


@pytest.mark.parametrize("n_vote", [0, 1, 2, 3, 4])
def test_hist_voting_frames(api, ro, n_vote):
    """N_FRAMES_HIST_VOTING 0..4 through test_assess_tracking_quality_parity's sequence of addOldPclAndPose /
    assessTrackingQuality / clearUpPastLists: histograms, overlaps, status and pastSize equal to the oracle's at every step;
    N <= 2 never asks for a keyframe (tracker.cpp:184: hsize < 4) on a sequence where N = 3 does.  N = 4: both vote with
    the OLDEST THREE past clouds, i.e. exactly like N = 3 (the reference would throw from histWeights.at(4), tracker.cpp:179)."""
    s = ImgPyramidSettings.scaled(320, 240, 3, **S320)
    pair = synth.make_pair(33, s)
    cam = api.CameraPyr(s)
    g_ref, g_cur = api.ImgPyramidRGBD(s, cam, *pair["ref"]), api.ImgPyramidRGBD(s, cam, *pair["curr"])
    o_ref, o_cur = ro.Pyramid(s, *pair["ref"]), ro.Pyramid(s, *pair["curr"])
    seq = {}
    for nv in sorted({n_vote, 3}):
        ts = TrackerSettings(n_frames_hist_voting=nv)
        gt = api.TrackerNew(ts, s, cam)
        assert gt.pastSize() == 0  # a new tracker on the same context starts with empty past lists (tracker.h:92-95)
        ot = ro.Tracker(s, OptimizerSettings(), ts)
        out = []
        for k, P in enumerate(VOTE_POSES):
            src_g, src_o = (g_ref, o_ref) if k % 2 == 0 else (g_cur, o_cur)
            gt.addOldPclAndPose(src_g, 2, P, float(k))
            ot.addOldPclAndPose(src_o, 2, P, float(k))
            if k == 3:
                gt.clearUpPastLists()
                ot.clearUpPastLists()
            for T in VOTE_QUERIES:
                st_g, h_g, o_g = gt.assessTrackingQuality(T, g_cur, return_hist=True)
                st_o, h_o, o_o = ot.assessTrackingQuality(T, o_cur)
                assert np.array_equal(h_g, h_o) and np.array_equal(o_g, o_o) and st_g == st_o, (nv, k, h_g, h_o, o_g, o_o)
                assert gt.pastSize() == ot.past_size()
                out.append((st_g, h_g.tolist(), o_g.tolist(), gt.pastSize()))
        seq[nv] = out
    assert max(o[3] for o in seq[3]) >= 4  # the past list grew beyond three clouds
    assert any(o[0] == TRACKER_STATE_NEW_KF for o in seq[3]), "the sequence must reach a keyframe vote at N = 3"
    if n_vote <= 2:
        assert all(o[0] != TRACKER_STATE_NEW_KF for o in seq[n_vote])
    if n_vote == 4:  # four past clouds, none cleared: N = 4 votes exactly like N = 3 (hsize 4, the oldest three clouds)
        got = []
        for nv in (3, 4):
            gt = api.TrackerNew(TrackerSettings(n_frames_hist_voting=nv), s, cam)
            for k, P in enumerate(VOTE_POSES[:4]):
                gt.addOldPclAndPose(g_ref if k % 2 == 0 else g_cur, 2, P, float(k))
            assert gt.pastSize() == 4
            got.append([(a, b.tolist(), c.tolist()) for a, b, c in
                        (gt.assessTrackingQuality(T, g_cur, return_hist=True) for T in VOTE_QUERIES)])
        assert got[0] == got[1]


def test_vo_at_the_orbbec_configuration(ro):
    """Sequential VO at orbbec_dataset's values (Canny 60/20, its intrinsics, u16 depth at 1000 through revo_vo_submit_u16),
    640x480 / 3 levels: the same keyframes as the oracle's REVO::start with the default tracker settings, with
    CHECK_TRACKING_RESULTS 0 (first frame only) and with N_FRAMES_HIST_VOTING 1; the IO-thread driver gives the same bits."""
    from revo_amd import vo
    name, kw, scale = [c for c in CONFIGS if "orbbec_dataset" in c[0]][0]
    assert scale == 1000.0 and (kw["canny_threshold1"], kw["canny_threshold2"]) == (60, 20)
    s = config_settings(kw, 3)
    n = 50
    frames = synth.make_sequence(12, s, n, max_t=0.01, max_rot_deg=0.4, bias=[0.004, 0, 0, 0, np.deg2rad(1.0), 0], workers=8)
    raws = [to_u16(f[1], scale) for f in frames]
    deps = [ro.u16_to_depth(r, scale) for r in raws]
    gt_poses = [f[3] for f in frames]
    for ts in (TrackerSettings(), TrackerSettings(check_tracking_results=0), TrackerSettings(n_frames_hist_voting=1)):
        gpu = vo.REVO(s, settingsTracker=ts, depth_scale_factor=scale)
        cpu = ro.VO(s, OptimizerSettings(), ts)
        est_g, est_o, kf_g, kf_o = [], [], [], []
        for i, f in enumerate(frames):
            pg, kg = gpu.push(f[0], raws[i], f[2])
            po, ko = cpu.push(f[0], deps[i], f[2])
            est_g.append(pg)
            est_o.append(po)
            kf_g += [i] if kg else []
            kf_o += [i] if ko else []
        d_rot = max(synth.rot_angle(a[:3, :3], b[:3, :3]) for a, b in zip(est_g, est_o))
        d_tr = max(float(np.linalg.norm(a[:3, 3] - b[:3, 3])) for a, b in zip(est_g, est_o))
        ate_go, ate_g = synth.ate_rmse(est_g, est_o), synth.ate_rmse(est_g, gt_poses)
        print("orbbec VO check=%d nvote=%d: keyframes %s / oracle %s, max diff %.2e rad %.2e m, ATE(gpu,oracle) %.2e, vs GT %.4f m"
              % (ts.check_tracking_results, ts.n_frames_hist_voting, kf_g, kf_o, d_rot, d_tr, ate_go, ate_g))
        assert kf_g == kf_o and gpu.nKeyFrames == cpu.num_keyframes(), (kf_g, kf_o)
        if ts.check_tracking_results and ts.n_frames_hist_voting == 3:
            assert len(kf_g) >= 3, kf_g  # the first frame and at least 2 keyframe changes
            assert ate_go < 1e-3 and d_rot < 5e-4 and d_tr < 5e-4
            assert ate_g < 0.01
        else:
            # no vote (CHECK_TRACKING_RESULTS 0: nvote = -1) or fewer than 3 voters (hsize < 4): never a new keyframe, so
            # the camera soon pans beyond what tracking against frame 0 can follow -- the bounds hold while it can
            assert kf_g == [0]
            k = 10
            assert synth.ate_rmse(est_g[:k], est_o[:k]) < 1e-3
            assert max(synth.rot_angle(a[:3, :3], b[:3, :3]) for a, b in zip(est_g[:k], est_o[:k])) < 5e-4
        if ts.n_frames_hist_voting == 3 and ts.check_tracking_results:
            gpu2 = vo.REVO(s, settingsTracker=ts, depth_scale_factor=scale, cameraPyr=gpu.camPyr)
            res2 = gpu2.run([(f[0], raws[i], f[2]) for i, f in enumerate(frames)])
            assert all(np.array_equal(a, b[0]) for a, b in zip(est_g, res2))
            assert [i for i, r in enumerate(res2) if r[1]] == kf_g
