"""The matrix of optimizer settings (tests/lm_settings_cases.py) without a GPU: in the oracle the cases reach the branches of the
LM loop they are there for (optimizer.cpp:235-311), the forced sequence lengths hold, the reference agrees with itself
(float against double sums) wherever the GPU tests compare against it, and the numpy restatements of the per-point terms
(tests/exact_sums_ref.py, tests/pair_info_ref.py) follow the Huber weight and the edge-distance filter away from the defaults."""
import math

import numpy as np
import pytest

from revo_amd.settings import PLANE_EDGES3D, PLANE_GRADTABLE

import exact_sums_ref as xr
import lm_settings_cases as lc
import pair_info_ref as pr

ALL = [(size, case, start) for size in ("160", "320") for case, start in lc.matrix(size)]
IDS = ["%s-%s-%s" % t for t in ALL]

# The ways a level can end under a case, beside the ones its settings rule out.  max_its 1 leaves no room for the ratio (the
# one accepted candidate is the cap); caps of 1-3 iterations from the coarsest level end before the error ratio passes 0.999;
# with the default cap of 100 the cap is never reached.
EXITS = {
    "gn1": {"cap", "small"},
    "cap3_nostep": {"cap", "conv", "small"},
    "caps123+smin": {"cap", "small"},
    "smin1e-6": {"conv", "small"},
    "smin1e-4": {"conv", "small"},
    "huber.05+smin": {"conv", "small"},
    "edist322+smin": {"conv", "small"},
    "edist1e9+smin": {"conv", "small"},
    "damped+cap3": {"cap", "conv", "small"},
    "damped+smin": {"conv", "small"},
    "damped2+smin": {"conv", "small"},
}


def _has_run_of_rejects(trace, n=2):
    run = 0
    for a in trace:
        run = 0 if a else run + 1
        if run >= n:
            return True
    return False


@pytest.mark.parametrize("case,start", lc.matrix("160"), ids=["%s-%s" % t for t in lc.matrix("160")])
def test_the_cases_exercise_the_branches(case, start):
    """160x120, the whole matrix, double sums: over the 16 pairs a candidate is rejected, two are rejected in a row (a retry
    chain longer than one pass of the shallowest speculation) -- except where step_size_min 1e30 rules retries out and for
    eps0 from the prior, which accepts nearly everything --, and every way the case's levels can end occurs.  (At 320x240 the
    reduced set rejects less: gn1 from the prior not once.  It is run for the lengths and the self-agreement below.)"""
    runs = lc.oracle_runs("160", case, start, True)
    os_ = lc.optimizer_settings(case)
    traces = [(lvl, t) for r in runs for lvl, t in enumerate(r["trace"])]
    assert all(r["flags"] == 0 for r in runs)
    assert sum(t.count(0) for _, t in traces) >= 1
    if case not in lc.NO_RETRIES and (case, start) != ("eps0", "prior"):
        assert any(_has_run_of_rejects(t) for _, t in traces)
    if case in lc.NO_RETRIES:
        assert not any(_has_run_of_rejects(t) for _, t in traces)
    if case in EXITS:
        seen = {lc.level_exit(t, os_.max_its_per_lvl[lvl]) for lvl, t in traces}
        assert seen >= EXITS[case], (seen, EXITS[case])


@pytest.mark.parametrize("size,case,start", [t for t in ALL if t[1] in lc.FORCED], ids=[i for t, i in zip(ALL, IDS) if t[1] in lc.FORCED])
def test_forced_lengths(size, case, start):
    """gn1: one candidate per level, accepted or not; cap3_nostep: at most three, the first rejected one ends the level;
    caps123+smin: one iteration at level 0, where a rejected candidate's step is below 1e-4.  Float and double sums."""
    for double in (False, True):
        for r in lc.oracle_runs(size, case, start, double):
            lc.check_forced_lengths(case, r["evals"])


@pytest.mark.parametrize("size,case,start", [t for t in ALL if t[1] != "free"], ids=[i for t, i in zip(ALL, IDS) if t[1] != "free"])
def test_the_reference_agrees_with_itself(size, case, start):
    """Float sums against double sums: identical evaluation counts on >= 15 of the 16 pairs, and there the poses within 1e-5
    (rotation angle and translation).  This is what lets the GPU tests hold the device to the double oracle under the case."""
    same, d_self = lc.self_distance(size, case, start)
    print("%s %s %s: equal counts %d/16, d_self %.3g" % (size, case, start, len(same), d_self))
    assert len(same) >= 15
    assert d_self <= 1e-5


def _ulps(a, b):
    def key(x):
        i = np.asarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


def test_restatements_follow_the_weights_and_the_filter():
    """exact_sums_ref.exact_eval and pair_info_ref.pair_info against the oracle's eval with double sums, under each Huber
    threshold and edge distance of WEIGHT_CASES with the filter on and off, on two 320x240 pairs at the identity, half the
    true translation and the tracked pose of every level: equal counts, every sum within 1 ulp and no more entries off by
    that ulp than test_exact_sums_cpu.py allows (8 in its 810).  Each setting changes the sums it should."""
    from oracle import ro
    s = lc.S320
    L = ro.lib()
    iu = np.triu_indices(6)
    n_entries = n_diff = worst = checked = n_fewer = 0
    L.ro_set_accum_double(1)
    try:
        conv_tracker = ro.Tracker(s, lc.optimizer_settings(None), lc.tracker_settings("id"))
        for p, (o_ref, o_cur) in list(zip(lc.pairs("320"), lc.oracle_pyramids("320")))[:2]:
            conv = conv_tracker.trackFrames(o_ref, o_cur, np.eye(3), np.zeros(3))
            gt = p["T_ref_curr"]
            poses = [(np.eye(3), np.zeros(3)), (gt[:3, :3], 0.5 * gt[:3, 3]), (conv["R"], conv["T"])]
            for lvl in range(s.nLevels()):
                args = (o_ref.read(PLANE_GRADTABLE, lvl), o_cur.read(PLANE_EDGES3D, lvl), o_ref.camera(lvl))
                for R, T in poses:
                    dflt = {}
                    for name in (None,) + tuple(lc.WEIGHT_CASES):
                        for filt in (1, 0):
                            os_ = lc.optimizer_settings(name, use_edge_filter=filt)
                            tail = (os_.edge_distance_lvl[lvl], os_.use_edge_filter, os_.huber_edge)
                            err_o, info, A_o, b_o = ro.Tracker(s, os_, lc.tracker_settings("id")).eval(o_ref, o_cur, R, T, lvl)
                            err, sw, su, good, bad, A, b = xr.exact_eval(*args, R, T, *tail)
                            rec = pr.record(pr.pair_info(*args, R, T, *tail, level=lvl))
                            where = (name, filt, lvl)
                            assert (good, bad) == (info.good_pts_edges, info.bad_pts_edges) == (rec.good, rec.bad), where
                            assert good > 50, where
                            if name is None:
                                dflt[filt] = (good, sw)
                                continue
                            ref = np.concatenate([np.asarray(A_o, np.float32)[iu], b_o,
                                                  np.array([info.sum_error_weighted, info.sum_error_unweighted, err_o], np.float32)])
                            n = np.float32(good)
                            for got in (np.concatenate([A[iu], b, [sw, su, err]]),
                                        np.concatenate([np.array(list(rec.H), np.float32) / n, -(np.array(list(rec.g), np.float32) / n),
                                                        [rec.sum_w, rec.sum_u, np.float32(rec.sum_w) / n]])):
                                d = _ulps(got, ref)
                                n_entries += len(d)
                                n_diff += int((d > 0).sum())
                                worst = max(worst, int(d.max()))
                            checked += 1
                            # the setting arrived: another weighted sum under another Huber threshold; under the tight
                            # edge distance never more good points and nearly always fewer; under 1e9 the filter removes
                            # nothing: the sums of the filter switched off (which on these scenes are the default's too --
                            # no residual lies above 30 / 20 / 10 --, so 1e9 cannot be told from the default by its counts);
                            # the filter off, the edge distance changes nothing
                            if name.startswith("huber"):
                                assert good == dflt[filt][0] and sw != dflt[filt][1], where
                            elif filt and name == "edist322":
                                assert good <= dflt[1][0], where
                                n_fewer += int(good < dflt[1][0])
                            else:
                                assert (good, sw.tobytes()) == (dflt[0][0], dflt[0][1].tobytes()), where
    finally:
        L.ro_set_accum_double(0)
    print("restatements vs double oracle: %d evaluations, %d of %d entries differ, at most %d ulp" % (checked, n_diff, n_entries, worst))
    assert checked == 2 * s.nLevels() * 3 * len(lc.WEIGHT_CASES) * 2
    assert n_fewer >= 9  # edist322 removed points at half of its 18 evaluations or more (one would show that it arrived)
    assert worst <= 1
    assert n_diff <= math.ceil(n_entries * 8 / 810)
