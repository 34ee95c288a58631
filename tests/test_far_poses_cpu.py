"""The far-pose cases of tests/far_pose_cases.py without a GPU: that the cases hold what test_gpu_far_poses.py relies on
(points behind the camera that count as good, poses that leave no valid point, projections exactly on the rims, priors the
initialisation check decides by a wide margin), and the numpy specification (tests/exact_sums_ref.py) against the
double-accumulating oracle at every one of them -- NaN where the reference divides 0 by 0 included."""
import numpy as np
import pytest

from revo_amd.settings import OptimizerSettings, TrackerSettings, PLANE_DT, PLANE_EDGES3D, PLANE_GRADTABLE

import exact_sums_ref as xr
import far_pose_cases as fc

OS = OptimizerSettings()


@pytest.fixture(scope="module")
def ro():
    from oracle import ro as R
    return R


def _pts(scene, lvl):
    return fc.oracle_pyramids(scene)[1].read(PLANE_EDGES3D, lvl)


def test_level_cameras_are_the_oracles():
    for scene in "AB":
        for lvl in range(fc.NLEVELS):
            assert tuple(fc.oracle_pyramids(scene)[0].camera(lvl)) == tuple(np.float32(c) for c in fc.level_camera(scene, lvl))


def test_rim_scene_projections_are_quarter_pixels_on_every_rim():
    """Scene B: Z = 2 on every point, every u, v of every shift a multiple of 1/4; at shift (0, 0) every level has points exactly
    on u = 1, u = w-2, v = 1 and v = h-2, and under the shifts by +-3 the cost function's u lands exactly on -1, 0, w-1 and w."""
    for lvl in range(fc.NLEVELS):
        cam = fc.level_camera("B", lvl)
        w, h = cam[4], cam[5]
        pts = _pts("B", lvl)
        assert len(pts) > 100 and np.all(pts[:, 2] == np.float32(fc.PLANE_Z))
        cost_u = []
        for kx, ky in fc.SHIFTS:
            R, T = fc.shift_pose(lvl, kx, ky)
            for cost in (False, True):
                u, v, _ = fc.projections(pts, cam, R, T, cost=cost)
                assert np.all(u * 4 == np.round(u * 4)) and np.all(v * 4 == np.round(v * 4)), (lvl, kx, ky, cost)
                if cost and (kx, ky) in ((3, 0), (-3, 0)):
                    cost_u.append(u)
            if (kx, ky) == (0, 0):
                n = [int((u == 1).sum()), int((u == w - 2).sum()), int((v == 1).sum()), int((v == h - 2).sum())]
                print("level %d: points on u = 1, u = w-2, v = 1, v = h-2: %s" % (lvl, n))
                assert min(n) >= 1, (lvl, n)
        cu = np.concatenate(cost_u)
        n = [int((cu == x).sum()) for x in (-1, 0, w - 1, w)]
        print("level %d: cost projections on u = -1, 0, w-1, w: %s" % (lvl, n))
        assert min(n) >= 1, (lvl, n)


def test_scene_a_holds_the_three_regimes():
    """Some pose has every Z < 0 and at least 80 % good points, some has good = 0 with a list that is not empty, some has 10-30 %
    good; the priors of EMPTY have good = 0 at every level."""
    ev = fc.oracle_evals("A")
    behind = empty = partial = 0
    for name, (R, T) in fc.poses_a().items():
        pts = _pts("A", 0)
        d = ev[(name, 0)][0]
        n = len(pts)
        assert d["good"] + d["bad"] == n
        z = fc.projections(pts, fc.level_camera("A", 0), R, T)[2]
        behind += bool(np.all(z < 0) and d["good"] >= 0.8 * n)
        empty += bool(d["good"] == 0 and n > 0)
        partial += bool(0.1 * n <= d["good"] <= 0.3 * n)
    assert behind >= 1 and empty >= 1 and partial >= 1, (behind, empty, partial)
    for name in fc.EMPTY:
        for lvl in range(fc.NLEVELS):
            d = ev[(name, lvl)][0]
            assert d["good"] == 0 and d["bad"] == len(_pts("A", lvl)) > 0 and np.isnan(d["err"]), (name, lvl)


def test_init_check_priors_are_decided_by_a_wide_margin(ro):
    """Every prior of the whole-tracker tests: |costInit - costEye| is at least 10 % of the larger (double sums).  EMPTY priors
    cost 0 and so beat the identity; BEATEN ones lose to it."""
    s = fc.SA
    o_ref, o_cur = fc.oracle_pyramids("A")
    ot = ro.Tracker(s, OS, TrackerSettings())
    L = ro.lib()
    L.ro_set_accum_double(1)
    try:
        c_eye = ot.eval_cost(np.eye(3), np.zeros(3), s.pyr_min_lvl, o_cur, o_ref)
        costs = {name: ot.eval_cost(*fc.poses_a()[name], s.pyr_min_lvl, o_cur, o_ref) for name in fc.EMPTY + fc.BEATEN}
    finally:
        L.ro_set_accum_double(0)
    print("costEye %.6g, costInit %s" % (c_eye, {k: round(float(v), 3) for k, v in costs.items()}))
    assert c_eye > 0
    for name, c in costs.items():
        assert abs(c - c_eye) >= 0.1 * max(c, c_eye), (name, c, c_eye)
        assert (c == 0) if name in fc.EMPTY else (c > c_eye), (name, c, c_eye)


def test_rim_priors_turn_on_each_rim_of_the_cost_function(ro):
    """far_pose_cases.RIM_RULES: under the reference's rule rim_cost is the oracle's cost and `costEye < costInit` its flag; with
    the one rim of the prior's name moved, the decision is the other one -- so a device that takes the oracle's decision at all
    five priors has every rim of `0 <= u < w && 0 <= v < h`, and the floor, where the reference has them."""
    lvl = fc.SB.pyr_min_lvl
    o_ref, o_cur = fc.oracle_pyramids("B")
    ot = ro.Tracker(fc.SB, OS, TrackerSettings())
    L = ro.lib()
    eye = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
    for rule, k in fc.RIM_RULES.items():
        R, T = fc.shift_pose(lvl, *k)
        L.ro_set_accum_double(1)
        try:
            c_eye, c_init = ot.eval_cost(*eye, lvl, o_cur, o_ref), ot.eval_cost(R, T, lvl, o_cur, o_ref)
            flag = ot.trackFrames(o_ref, o_cur, R, T)["flags"] & 1
        finally:
            L.ro_set_accum_double(0)
        assert (np.float32(fc.rim_cost(lvl, *eye)), np.float32(fc.rim_cost(lvl, R, T))) == (c_eye, c_init), rule
        assert c_eye != c_init and flag == int(c_eye < c_init), (rule, c_eye, c_init)
        wrong = int(fc.rim_cost(lvl, *eye, rule=rule) < fc.rim_cost(lvl, R, T, rule=rule))
        assert wrong != flag, (rule, flag, fc.rim_cost(lvl, *eye, rule=rule), fc.rim_cost(lvl, R, T, rule=rule))


def test_the_oracle_from_the_far_priors(ro):
    """What test_gpu_far_poses.py expects of the device, stated by the oracle: an EMPTY prior ends with flags 0, evals [2, 2, 2],
    a NaN error, good 0 / bad n, status NEW_KF and the prior's pose (T to the bit, R through the quaternion and back), with the
    check on and off and with float and double sums; a BEATEN prior with the check on is the identity start with flag bit 0."""
    n0 = len(_pts("A", 0))
    for double in (False, True):
        eye = fc.oracle_track("identity", 1, double)
        assert eye["flags"] == 0 and np.isfinite(eye["err"])
        for chk in (1, 0):
            for name in fc.EMPTY:
                r = fc.oracle_track(name, chk, double)
                R, T = fc.poses_a()[name]
                assert (r["flags"], r["evals"], r["good"], r["bad"], r["status"]) == (0, (2, 2, 2), 0, n0, 2), (name, chk, r)
                assert np.isnan(r["err"]) and r["T"].tobytes() == T.tobytes() and np.abs(r["R"] - R).max() <= 1e-6, (name, chk, r)
        for name in fc.BEATEN:
            r = fc.oracle_track(name, 1, double)
            assert r["flags"] == 1 and r["evals"] == eye["evals"] and r["err"] == eye["err"], (name, r)
            assert r["R"].tobytes() == eye["R"].tobytes() and r["T"].tobytes() == eye["T"].tobytes(), name


def test_spec_against_the_double_oracle_at_every_far_pose(ro):
    """exact_sums_ref.exact_eval against ro_set_accum_double(1) for every case and level of both scenes: good / bad equal, A, b,
    the two error sums and the mean error within 1 ulp (test_restatement_matches_the_double_accumulating_oracle's bar), NaN
    exactly where the oracle has NaN."""
    worst = n_entries = n_diff = n_nan = 0
    iu = np.triu_indices(6)
    for scene in "AB":
        o_ref, o_cur = fc.oracle_pyramids(scene)
        ev = fc.oracle_evals(scene)
        for name, lvl, R, T in fc.cases(scene):
            o = ev[(name, lvl)][0]
            err, sw, su, good, bad, A, b = xr.exact_eval(o_ref.read(PLANE_GRADTABLE, lvl), o_cur.read(PLANE_EDGES3D, lvl), o_ref.camera(lvl),
                                                         R, T, OS.edge_distance_lvl[lvl], OS.use_edge_filter, OS.huber_edge)
            where = (scene, name, lvl)
            assert (good, bad) == (o["good"], o["bad"]), where
            got = np.concatenate([A[iu], b, [sw, su, err]]).astype(np.float32)
            ref = np.concatenate([o["A"][iu], o["b"], [o["sum_w"], o["sum_u"], o["err"]]]).astype(np.float32)
            assert np.array_equal(np.isnan(got), np.isnan(ref)), (where, got, ref)
            assert np.isnan(got).any() == (good == 0), where
            ok = ~np.isnan(got)
            d = fc.ulps(got[ok], ref[ok])
            n_nan += int((~ok).sum())
            n_entries += len(d)
            n_diff += int((d > 0).sum())
            worst = max(worst, int(d.max()))
            assert d.max() <= 1, (where, d)
            if good == 0:  # the sums themselves are +0
                assert sw.tobytes() == su.tobytes() == np.float32(0).tobytes() == o["sum_w"].tobytes() == o["sum_u"].tobytes(), where
    print("spec vs double oracle at far poses: %d of %d entries differ, at most %d ulp; %d NaN entries" % (n_diff, n_entries, worst, n_nan))
    assert n_nan == 28 * 2 * fc.NLEVELS  # A, b and the mean error of the two empty poses; their two sums are 0


def test_cost_function_spec_against_the_oracle(ro):
    """exact_sums_ref.eval_cost is ro_tracker_eval_cost (double sums) at every case and level, rim shifts included, bit for bit."""
    L = ro.lib()
    n_zero = 0
    for scene in "AB":
        o_ref, o_cur = fc.oracle_pyramids(scene)
        ot = ro.Tracker(fc.settings(scene), OS, TrackerSettings())
        for name, lvl, R, T in fc.cases(scene):
            L.ro_set_accum_double(1)
            try:
                want = np.float32(ot.eval_cost(R, T, lvl, o_cur, o_ref))
            finally:
                L.ro_set_accum_double(0)
            got = xr.eval_cost(o_ref.read(PLANE_DT, lvl), o_cur.read(PLANE_EDGES3D, lvl), o_ref.camera(lvl), R, T,
                               OS.edge_distance_lvl[lvl], OS.use_edge_filter)
            assert got.tobytes() == want.tobytes(), (scene, name, lvl, got, want)
            n_zero += int(want == 0)
    assert n_zero >= 2 * fc.NLEVELS
