"""The exact-sums mode without a GPU: its specification (tests/exact_sums_ref.py, the reference's per-point float terms and the
float nearest their exact sum) against the double-accumulating oracle, the new C ABI symbols, and run_tum --exact-sums."""
import numpy as np
import pytest

from revo_amd import synth
from revo_amd.settings import ImgPyramidSettings, OptimizerSettings, TrackerSettings, PLANE_EDGES3D, PLANE_GRADTABLE

import exact_sums_ref as xr


def _ulps(a, b):
    """Distance in float32 units in the last place (same-sign ordering of the bit patterns)."""
    def key(x):
        i = np.asarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


def test_round_exact_f32_ties_and_cancellation():
    big = np.float32(2.0 ** 24)
    # 2^24 + 1 is a float midpoint: ties to even (2^24), the tiny third term pushes it up (2^24 + 2)
    assert xr.round_exact_f32([big, np.float32(1)]) == big
    assert xr.round_exact_f32([big, np.float32(1), np.float32(2.0 ** -30)]) == np.float32(2.0 ** 24 + 2)
    # a sum whose double rounding lands on the midpoint while the exact value lies just above it
    terms = np.array([1.0, 2.0 ** -24, 2.0 ** -80, 2.0 ** -80], np.float32)
    assert xr.round_exact_f32(terms) == np.nextafter(np.float32(1), np.float32(2))
    # total cancellation: +0
    r = xr.round_exact_f32([np.float32(3.5), np.float32(-3.5)])
    assert r == 0 and not np.signbit(r)


@pytest.fixture(scope="module")
def pairs():
    s = ImgPyramidSettings.scaled(320, 240, 3, hist_patch=(10, 5, 0, 0, 0, 0))
    return s, [synth.make_pair(seed, s) for seed in (31, 32, 33)]


def test_restatement_matches_the_double_accumulating_oracle(pairs):
    """The restatement against ro_set_accum_double(1) (the reference's terms, summed in double in list order, rounded once):
    the exact and the double-sequential sums round to the same float on all but a handful of the entries, never more than 1 ulp
    apart -- at the initial, a mid-way and the converged pose of every level (the converged ones are where b cancels)."""
    from oracle import ro
    s, prs = pairs
    os_ = OptimizerSettings()
    ot = ro.Tracker(s, os_, TrackerSettings())
    L = ro.lib()
    n_entries = n_diff = 0
    worst = 0
    checked = 0
    L.ro_set_accum_double(1)
    try:
        for p in prs:
            o_ref, o_cur = ro.Pyramid(s, *p["ref"]), ro.Pyramid(s, *p["curr"])
            o_ref.makeKeyframe()
            conv = ot.trackFrames(o_ref, o_cur, np.eye(3), np.zeros(3))
            gt = p["T_ref_curr"]
            poses = [(np.eye(3), np.zeros(3)), (gt[:3, :3], 0.5 * gt[:3, 3]), (conv["R"], conv["T"])]
            for lvl in range(s.nLevels()):
                tab = o_ref.read(PLANE_GRADTABLE, lvl)
                pts = o_cur.read(PLANE_EDGES3D, lvl)
                cam = o_ref.camera(lvl)
                for R, T in poses:
                    err_o, info, A_o, b_o = ot.eval(o_ref, o_cur, R, T, lvl)
                    err, sw, su, good, bad, A, b = xr.exact_eval(tab, pts, cam, R, T, os_.edge_distance_lvl[lvl],
                                                                os_.use_edge_filter, os_.huber_edge)
                    assert (good, bad) == (info.good_pts_edges, info.bad_pts_edges)
                    assert good > 50
                    iu = np.triu_indices(6)
                    got = np.concatenate([A[iu], b, [sw, su, err]])
                    ref = np.concatenate([np.asarray(A_o, np.float32)[iu], b_o,
                                          np.array([info.sum_error_weighted, info.sum_error_unweighted, err_o], np.float32)])
                    d = _ulps(got, ref)
                    n_entries += len(d)
                    n_diff += int((d > 0).sum())
                    worst = max(worst, int(d.max()))
                    checked += 1
    finally:
        L.ro_set_accum_double(0)
    print("restatement vs double oracle: %d evaluations, %d of %d entries differ, at most %d ulp" % (checked, n_diff, n_entries, worst))
    assert checked == len(prs) * s.nLevels() * 3
    assert worst <= 1
    assert n_diff <= 8


def test_exact_sums_symbols_are_declared_and_exported():
    from revo_amd import _lib
    syms = _lib.declared_symbols()
    for name in ("revo_ctx_set_exact_sums", "revo_ctx_exact_sums"):
        assert name in syms
        assert hasattr(_lib.lib(), name)


class _Stop(Exception):
    pass


def _yaml(tmp_path):
    (tmp_path / "dataset.yaml").write_text(
        "%%YAML:1.0\nCamera.fx: 300.0\nCamera.fy: 300.0\nCamera.cx: 160.0\nCamera.cy: 120.0\nCamera.width: 320\n"
        "Camera.height: 240\nwidth: 320\nheight: 240\nMainFolder: \"%s/\"\nDatasets: [\"a\", \"b\"]\n"
        "ASSOCIATE: \"associate.txt\"\nPYR_MIN_LVL: 2\nPYR_MAX_LVL: 0\nDEPTH_SCALE_FACTOR: 5000.0\n" % str(tmp_path))
    (tmp_path / "settings.yaml").write_text("%YAML:1.0\nCHECK_TRACKING_RESULTS: 1\nCHECK_INIT_VALUES: 1\nUSE_EDGE_FILTER: 1\n"
                                            "N_FRAMES_HIST_VOTING: 3\nDO_OUTPUT_POSES: 1\n")
    return [str(tmp_path / "settings.yaml"), str(tmp_path / "dataset.yaml")]


@pytest.mark.parametrize("extra", [[], ["--exact-sums"], ["--streams", "2"], ["--streams", "2", "--exact-sums"],
                                   ["--exact-sums", "--streams", "3", "--decoders", "0"]])
def test_run_tum_exact_sums_reaches_the_driver(tmp_path, monkeypatch, extra):
    """--exact-sums is taken out of the argument list and handed to the context the sequential loop creates / to
    vo.MultiREVO; without it both get exact_sums=False."""
    from revo_amd import api, run_tum, vo
    seen = {}

    def fake_cam(*a, **k):
        seen["cam"] = k.get("exact_sums", False)
        raise _Stop()

    def fake_multi(*a, **k):
        seen["multi"] = k.get("exact_sums", False)
        raise _Stop()

    monkeypatch.setattr(api, "CameraPyr", fake_cam)
    monkeypatch.setattr(vo, "MultiREVO", fake_multi)
    with pytest.raises(_Stop):
        run_tum.main(_yaml(tmp_path) + extra)
    want = "--exact-sums" in extra
    assert seen == ({"multi": want} if "--streams" in extra else {"cam": want})


def test_run_tum_exact_sums_keeps_the_argument_checks(capsys):
    from revo_amd import run_tum
    assert run_tum.main(["settings.yaml", "dataset.yaml", "--exact-sums", "--streams", "0"]) == 2
    assert "positive number of streams" in capsys.readouterr().out
    assert run_tum.main(["settings.yaml", "dataset.yaml", "--exact-sums", "--gpu-decode"]) == 2
