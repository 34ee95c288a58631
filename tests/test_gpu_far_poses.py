"""The tracker's per-point rules on the MI355X at poses far from the truth (tests/far_pose_cases.py): the cloud behind the camera
(the reference has no Z > 0 test), poses that leave no valid point although the list is not empty (0 / 0 through the LM ladder),
and projections exactly on the rims of the validity test and of the cost function.

a. revo_tracker_pair_info: the 192 bytes of pair_info_ref.pair_info at every case.
b. Exact-sums context, Optimizer.evalAt: exact_sums_ref.exact_eval bit for bit, NaN where the specification has NaN.
c. Default context, evalAt: the counts are the specification's; error, A and b lie within max(bar, 4 d_self) of the double-sum
   oracle, bar = test_residual_and_normal_equations_parity's and d_self = the oracle's own float-against-double distance.
d. The whole tracker from far priors, the single-pair call and one batch holding all priors.
e. revo_batch_pair_info with one pose per pair: the bytes of the single call.
f. The quality vote with a half turn and the through pose among the stored clouds."""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from revo_amd import synth  # noqa: E402
from revo_amd.settings import OptimizerSettings, TrackerSettings, PLANE_EDGES3D, PLANE_GRADTABLE  # noqa: E402

import exact_sums_ref as xr  # noqa: E402
import far_pose_cases as fc  # noqa: E402
import pair_info_ref as pr  # noqa: E402

KNOBS = ("REVO_TRACK_CLUSTER", "REVO_TRACK_CLUSTER_ONE", "REVO_TRACK_REDUNDANT_BATCH", "REVO_TRACK_REDUNDANT_ONE",
         "REVO_TRACK_KSPEC", "REVO_TRACK_KSPEC_ONE")
REC, INFO = 96, 192  # sizeof(revo_pair_result), sizeof(revo_pair_info)
FLAGS_AT = 88        # offsetof(revo_pair_result, flags)
ROT_TOL = 1e-4       # rad, test_gpu_parity.py's
TRANS_TOL = 1e-4     # m
MAX_TOTAL_EVALS = 6000  # k_track's cap (flag bit 2)
NEW_KF = 2
OS = OptimizerSettings()
MODES = [pytest.param(True, id="exact"), pytest.param(False, id="float")]
# two of test_gpu_exact_sums.PARTITIONS beside the shipped knobs: one cluster > 1, one speculation depth 4
PARTITIONS = [("shipped", {}), ("c2", {"REVO_TRACK_CLUSTER": "2", "REVO_TRACK_CLUSTER_ONE": "2"}),
              ("k4", {"REVO_TRACK_KSPEC": "4", "REVO_TRACK_KSPEC_ONE": "4"})]


def _clear(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _frames(cam, scene):
    from revo_amd import api
    s, p = fc.settings(scene), fc.pair(scene)
    ref = api.ImgPyramidRGBD(s, cam, *p["ref"])
    cur = api.ImgPyramidRGBD(s, cam, *p["curr"])
    ref.makeKeyframe()
    return ref, cur


@functools.lru_cache(maxsize=None)
def _dev(scene, exact):
    """(cam, trk, ref, cur) under the default settings; created by tests that have cleared the knobs.  Do not change its settings."""
    from revo_amd import api
    cam = api.CameraPyr(fc.settings(scene), exact_sums=exact)
    trk = api.TrackerNew(TrackerSettings(), fc.settings(scene), cam)
    return (cam, trk) + _frames(cam, scene)


@functools.lru_cache(maxsize=None)
def _spec(scene):
    """{(name, lvl): (exact_eval's tuple, pair_info's bytes)} from the device's own table and list, which are the oracle's.
    Computed once per scene; do not modify."""
    cam, _, ref, cur = _dev(scene, False)
    o_ref, o_cur = fc.oracle_pyramids(scene)
    out = {}
    for lvl in range(fc.NLEVELS):
        tab, pts = ref.returnOptimizationStructure(lvl), cur.return3DEdges(lvl)
        assert np.array_equal(tab, o_ref.read(PLANE_GRADTABLE, lvl)) and np.array_equal(pts, o_cur.read(PLANE_EDGES3D, lvl)), (scene, lvl)
        c = cam.at(lvl)
        c6 = (c.fx, c.fy, c.cx, c.cy, c.width, c.height)
        assert c6 == tuple(fc.level_camera(scene, lvl))
        tail = (OS.edge_distance_lvl[lvl], OS.use_edge_filter, OS.huber_edge)
        for name, l, R, T in fc.cases(scene):
            if l == lvl:
                out[(name, lvl)] = (xr.exact_eval(tab, pts, c6, R, T, *tail), pr.pair_info(tab, pts, c6, R, T, *tail, level=lvl))
    return out


@functools.lru_cache(maxsize=None)
def _single_infos(scene):
    """{(name, lvl): bytes of revo_tracker_pair_info}.  Do not modify."""
    _, trk, ref, cur = _dev(scene, False)
    return {(name, lvl): bytes(trk.pairInfo(ref, cur, R, T, lvl)) for name, lvl, R, T in fc.cases(scene)}


def _same_bits(got, want):
    """Equal bit for bit, except that where `want` is NaN any NaN will do."""
    got, want = np.asarray(got, np.float32).ravel(), np.asarray(want, np.float32).ravel()
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and got[~nan].tobytes() == want[~nan].tobytes()


@pytest.mark.parametrize("scene", ["A", "B"])
def test_pair_info_is_the_specification_at_every_far_pose(monkeypatch, scene):
    """a. Every case and level: the 192 bytes of pair_info_ref.pair_info.  Where no point is valid that is all sums +0 and
    bad = n; behind the camera the points count as good."""
    _clear(monkeypatch)
    spec, got = _spec(scene), _single_infos(scene)
    n_empty = n_behind = 0
    for name, lvl, R, T in fc.cases(scene):
        want = spec[(name, lvl)][1]
        g, w = np.frombuffer(got[(name, lvl)], np.float32), np.frombuffer(want, np.float32)
        rec = pr.record(got[(name, lvl)])
        assert got[(name, lvl)] == want, (scene, name, lvl, rec.good, rec.bad, pr.record(want).good, pr.record(want).bad, g[:29] - w[:29])
        if rec.good == 0:
            assert rec.bad > 0 and rec.flags == 0 and not any(got[(name, lvl)][:116]), (name, lvl)  # H, g, sum_w, sum_u: +0
            n_empty += 1
        n_behind += int(name in ("yaw180", "behind") and rec.good >= 0.8 * (rec.good + rec.bad))  # every Z < 0 under both
    assert (n_empty, n_behind) == ((2 * fc.NLEVELS, 2 * fc.NLEVELS) if scene == "A" else (0, 0))


@pytest.mark.parametrize("scene", ["A", "B"])
def test_exact_eval_is_the_specification_at_every_far_pose(monkeypatch, scene):
    """b. Exact-sums context: evalAt's error, sums, A, b and counts are exact_eval's bit for bit; where the specification has
    NaN (no valid point: 0 / 0) the device has NaN."""
    _clear(monkeypatch)
    spec = _spec(scene)
    cam, trk, ref, cur = _dev(scene, True)
    assert cam.exact_sums
    for name, lvl, R, T in fc.cases(scene):
        e_x, sw, su, good, bad, A_x, b_x = spec[(name, lvl)][0]
        err, info, A, b = trk.mOptimizer.evalAt(ref, cur, R, T, lvl)
        where = (scene, name, lvl)
        assert (info.good_pts_edges, info.bad_pts_edges) == (good, bad), where
        assert np.float32(info.sum_error_weighted).tobytes() == sw.tobytes(), where
        assert np.float32(info.sum_error_unweighted).tobytes() == su.tobytes(), where
        assert _same_bits(err, e_x), (where, err, e_x)
        assert _same_bits(A, A_x), (where, A - A_x)
        assert _same_bits(b, b_x), (where, b - b_x)
        assert bool(np.isnan(err)) == (good == 0), where


@pytest.mark.parametrize("scene", ["A", "B"])
def test_default_eval_against_the_double_oracle_at_every_far_pose(monkeypatch, capsys, scene):
    """c. Default context: good / bad are the specification's (integers: no order of summation moves them); error, A and b lie
    within max(bar, 4 d_self) of the double-sum oracle in far_pose_cases.scaled_distance's norm -- bar = 1e-5 on the error and
    1e-4 on A and b (test_residual_and_normal_equations_parity), d_self the oracle's float-against-double distance at the same
    case (the rule test_gpu_optimizer_settings.py applies to poses).  Where no point is valid all three are NaN."""
    _clear(monkeypatch)
    spec, ev = _spec(scene), fc.oracle_evals(scene)
    cam, trk, ref, cur = _dev(scene, False)
    assert not cam.exact_sums
    lines, bad_cases = [], []
    for name, lvl, R, T in fc.cases(scene):
        good, bad = spec[(name, lvl)][0][3:5]
        o = ev[(name, lvl)][0]
        err, info, A, b = trk.mOptimizer.evalAt(ref, cur, R, T, lvl)
        where = (scene, name, lvl)
        assert (info.good_pts_edges, info.bad_pts_edges) == (good, bad) == (o["good"], o["bad"]), where
        if good == 0:
            assert np.isnan(err) and np.all(np.isnan(A)) and np.all(np.isnan(b)), where
            assert info.sum_error_weighted == 0 and info.sum_error_unweighted == 0, where
            continue
        ds = fc.d_self(scene, name, lvl)
        d = fc.scaled_distance(dict(err=np.float32(err), A=np.asarray(A, np.float32), b=np.asarray(b, np.float32)), o)
        tol = tuple(max(bar, 4.0 * x) for bar, x in zip((1e-5, 1e-4, 1e-4), ds))
        lines.append("| %s | %s | %d | %d | %.2e %.2e %.2e | %.2e %.2e %.2e |" % ((scene, name, lvl, good) + d + ds))
        if not all(x <= t for x, t in zip(d, tol)):
            bad_cases.append((where, d, ds, tol))
    with capsys.disabled():
        print("\n| scene | case | level | good | device to double oracle: err A b | d_self: err A b |\n" + "\n".join(lines))
    assert not bad_cases, bad_cases


def _batch(cam, scene, n):
    """n pairs, every one the scene's two frames, built once -> (BatchTracker, the buffers it reads)"""
    import torch
    from revo_amd import api
    p = fc.pair(scene)
    bgr = torch.from_numpy(np.stack([p[k][0] for _ in range(n) for k in ("ref", "curr")])).cuda()
    dep = torch.from_numpy(np.stack([p[k][1] for _ in range(n) for k in ("ref", "curr")])).cuda()
    bt = api.BatchTracker(cam, n)
    bt.build(bgr.data_ptr(), dep.data_ptr())
    bt.sync()
    return bt, (bgr, dep)


def _track(bt, poses):
    """track_only from one prior per pair -> raw records"""
    import torch
    from revo_amd import api
    n = len(poses)
    d_res = torch.zeros(n * REC, dtype=torch.uint8, device="cuda")
    bt.track_only(d_res.data_ptr(), init_RT=api.pack_init_RT([R for R, _ in poses], [T for _, T in poses]))
    bt.sync()
    buf = d_res.cpu().numpy().tobytes()
    return [buf[i * REC:(i + 1) * REC] for i in range(n)]


def _records(raw):
    from revo_amd import api
    return api.results_from_buffer(b"".join(raw), len(raw))


def _check_empty(name, R, T, err, good, bad, status, evals, n0):
    """What the oracle reports from a prior that leaves no valid point (test_far_poses_cpu.py pins the oracle to it)."""
    R0, T0 = fc.poses_a()[name]
    assert tuple(int(e) for e in evals[:3]) == (2, 2, 2) and all(e == 0 for e in evals[3:]), (name, evals)
    assert np.isnan(err) and (good, bad, status) == (0, n0, NEW_KF), (name, err, good, bad, status)
    assert np.asarray(T, np.float32).tobytes() == T0.tobytes(), (name, T)
    # the rotation went through the quaternion and back, as in the reference: a few ulp of 1; the identity comes back exactly
    assert np.abs(np.asarray(R, np.float32) - R0).max() <= 1e-6, (name, R)
    if np.array_equal(R0, np.eye(3)):
        assert np.asarray(R, np.float32).tobytes() == R0.tobytes(), (name, R)


@pytest.mark.parametrize("exact", MODES)
def test_a_prior_without_a_valid_point_ends_like_the_oracle(monkeypatch, exact):
    """d. Priors that give good = 0 at every level (a quarter turn, T = (1000, 0, 0)), with check_init_values 1 and 0: the
    initialisation check gives such a prior the cost 0, so it beats the identity, and the ladder runs on NaN errors -- flags 0,
    evals [2, 2, 2], err NaN, the pose of the prior, good 0 / bad n, status NEW_KF, from the single-pair call and from a batch."""
    from revo_amd import api
    _clear(monkeypatch)
    cam = api.CameraPyr(fc.SA, exact_sums=exact)
    ref, cur = _frames(cam, "A")
    n0 = cur.return3DEdges(0).shape[0]
    bt, keep = _batch(cam, "A", len(fc.EMPTY))
    for chk in (1, 0):
        trk = api.TrackerNew(TrackerSettings(check_init_values=chk), fc.SA, cam)
        for name in fc.EMPTY:
            o = fc.oracle_track(name, chk, True)
            assert (o["flags"], o["evals"], o["good"], o["bad"], o["status"]) == (0, (2, 2, 2), 0, n0, NEW_KF) and np.isnan(o["err"])
            status, R, T, err = trk.trackFrames(*fc.poses_a()[name], ref, cur)
            _check_empty(name, R, T, err, trk.last_info.good_pts_edges, trk.last_info.bad_pts_edges, status, trk.last_evals, n0)
        for name, r in zip(fc.EMPTY, _records(_track(bt, [fc.poses_a()[n] for n in fc.EMPTY]))):
            assert r["flags"] == 0, (name, chk, r["flags"])
            _check_empty(name, r["R"], r["T"], r["err"], r["good"], r["bad"], r["status"], r["evals"], n0)


@pytest.mark.parametrize("exact", MODES)
def test_priors_the_identity_beats_are_identity_starts(monkeypatch, exact):
    """d. One batch holding every prior of far_pose_cases.PRIORS on the same two frames, and the single-pair call, with the check on.
    Exact mode: the record of a beaten prior is the identity start's byte for byte, with flags bit 0 set.  Default mode: the
    flag is the oracle's and the pose lies within ROT_TOL / TRANS_TOL of the oracle's.  The priors without a valid point keep
    their pose among them."""
    from revo_amd import api
    _clear(monkeypatch)
    cam = api.CameraPyr(fc.SA, exact_sums=exact)
    trk = api.TrackerNew(TrackerSettings(check_init_values=1), fc.SA, cam)
    ref, cur = _frames(cam, "A")
    n0 = cur.return3DEdges(0).shape[0]
    bt, keep = _batch(cam, "A", len(fc.PRIORS))
    raw = _track(bt, [fc.poses_a()[n] for n in fc.PRIORS])
    recs = dict(zip(fc.PRIORS, _records(raw)))
    raw = dict(zip(fc.PRIORS, raw))

    def single(name):
        status, R, T, err = trk.trackFrames(*fc.poses_a()[name], ref, cur)
        return (np.asarray(R, np.float32).tobytes(), np.asarray(T, np.float32).tobytes(), np.float32(err).tobytes(),
                trk.last_info.good_pts_edges, trk.last_info.bad_pts_edges, status, tuple(trk.last_evals.tolist()))

    eye = single("identity")
    assert recs["identity"]["flags"] == 0 and recs["identity"]["good"] > 0.9 * n0
    for name in fc.BEATEN:
        o = fc.oracle_track(name, 1)
        r = recs[name]
        assert o["flags"] == 1 and r["flags"] == o["flags"], (name, r["flags"])
        if exact:
            want = bytearray(raw["identity"])
            want[FLAGS_AT:FLAGS_AT + 4] = np.int32(1).tobytes()
            assert raw[name] == bytes(want), name
            assert single(name) == eye, name
        else:
            status, R, T, err = trk.trackFrames(*fc.poses_a()[name], ref, cur)
            for Rg, Tg in ((R, T), (r["R"], r["T"])):
                assert synth.rot_angle(Rg, o["R"]) < ROT_TOL and np.linalg.norm(Tg - o["T"]) < TRANS_TOL, name
            assert status == o["status"] == r["status"], name
    for name in fc.EMPTY:
        r = recs[name]
        assert r["flags"] == 0, name
        _check_empty(name, r["R"], r["T"], r["err"], r["good"], r["bad"], r["status"], r["evals"], n0)


@functools.lru_cache(maxsize=None)
def _mixed_runs(chk):
    """Exact mode, every prior of PRIORS on scene A's frames with check_init_values = chk, under each of PARTITIONS (a fresh
    context each): {label: (records of ONE batch holding all priors, the record of each prior alone in a batch of one,
    the single-pair call's (R, T, err, good, bad, status, evals))}.  Do not modify."""
    from revo_amd import api
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    out = {}
    try:
        for label, env in PARTITIONS:
            os.environ.update(env)
            try:
                cam = api.CameraPyr(fc.SA, exact_sums=True)
                trk = api.TrackerNew(TrackerSettings(check_init_values=chk), fc.SA, cam)
                ref, cur = _frames(cam, "A")
                poses = [fc.poses_a()[n] for n in fc.PRIORS]
                bt, keep = _batch(cam, "A", len(poses))
                together = _track(bt, poses)
                b1, keep1 = _batch(cam, "A", 1)
                alone = [_track(b1, [p])[0] for p in poses]
                singles = []
                for R0, T0 in poses:
                    status, R, T, err = trk.trackFrames(R0, T0, ref, cur)
                    singles.append((np.asarray(R, np.float32).tobytes(), np.asarray(T, np.float32).tobytes(), np.float32(err).tobytes(),
                                    trk.last_info.good_pts_edges, trk.last_info.bad_pts_edges, status, tuple(trk.last_evals.tolist())))
                out[label] = (together, alone, singles)
                del bt, b1, keep, keep1, ref, cur, trk, cam
            finally:
                for k in env:
                    os.environ.pop(k, None)
    finally:
        for k, v in saved.items():
            if v is not None:
                os.environ[k] = v
    return out


def _key(r):
    return (r["R"].tobytes(), r["T"].tobytes(), np.float32(r["err"]).tobytes(), r["good"], r["bad"], r["status"], tuple(r["evals"].tolist()))


@pytest.mark.parametrize("chk", [1, 0])
def test_a_nan_pair_does_not_reach_its_neighbours(chk):
    """d. The mixed batch in exact mode: every pair's record is the record that pair gives in a batch of its own, in bytes, and the
    single-pair call reports the same pose, error, counts, status and evaluations -- the two NaN pairs sit between an identity
    start and priors that wander (check off) or are reset (check on).  Under the shipped knobs, a cluster of 2 and a
    speculation depth of 4; the records of the three are the same bytes."""
    runs = _mixed_runs(chk)
    base = runs[PARTITIONS[0][0]][0]
    for label, (together, alone, singles) in runs.items():
        diff = [n for n, a, b in zip(fc.PRIORS, together, alone) if a != b]
        assert not diff, (label, "batch of its own", diff)
        diff = [n for n, r, k in zip(fc.PRIORS, _records(together), singles) if _key(r) != k]
        assert not diff, (label, "single-pair call", diff)
        diff = [n for n, a, b in zip(fc.PRIORS, together, base) if a != b]
        assert not diff, (label, "partition", diff)
    recs = dict(zip(fc.PRIORS, _records(base)))
    for name in fc.EMPTY:
        assert np.isnan(recs[name]["err"]) and recs[name]["good"] == 0
    assert np.isfinite(recs["identity"]["err"])


def test_far_priors_with_the_check_off_stay_within_the_caps():
    """d. Check off, priors yaw 180 / yaw 45 / through: the two sides walk different ways through a far landscape, so there is no
    pose parity with the oracle.  The exact-mode bytes are equal across the partitions (test_a_nan_pair_does_not_reach_its_
    neighbours[0]), good + bad = n, every level was evaluated, the evaluation cap was not hit and no flag is set."""
    runs = _mixed_runs(0)
    n0 = len(fc.oracle_pyramids("A")[1].read(PLANE_EDGES3D, 0))
    recs = {label: dict(zip(fc.PRIORS, _records(together))) for label, (together, _, _) in runs.items()}
    raws = {label: dict(zip(fc.PRIORS, together)) for label, (together, _, _) in runs.items()}
    for name in fc.WANDER:
        for label in recs:
            r = recs[label][name]
            assert raws[label][name] == raws[PARTITIONS[0][0]][name], (name, label)
            assert r["good"] + r["bad"] == n0 and r["flags"] == 0, (name, label, r)
            ev = r["evals"].tolist()
            assert all(e >= 1 for e in ev[:3]) and all(e == 0 for e in ev[3:]) and sum(ev) <= MAX_TOTAL_EVALS, (name, label, ev)
            assert np.all(np.isfinite(r["R"])) and np.all(np.isfinite(r["T"])), (name, label)
        print("check off, %s: evals %s, good %d, oracle evals %s" % (name, recs[PARTITIONS[0][0]][name]["evals"][:3].tolist(),
                                                                     recs[PARTITIONS[0][0]][name]["good"], fc.oracle_track(name, 0, True)["evals"]))


def test_rim_shift_priors_decide_like_the_oracle(monkeypatch):
    """d, the cost function's rule: the rim scene's shifts of the coarsest level as priors (the shifts by +-3 put points exactly
    on u = -1, 0, w-1 and w there), and the five priors of far_pose_cases.RIM_RULES, at each of which the decision turns over
    as soon as one rim of `0 <= u < w && 0 <= v < h`, or the floor, is moved (test_far_poses_cpu.py).  The device does not report
    the cost; both sides sum the distance-transform terms exactly (floats of a few bits in double), so flags bit 0 is the
    oracle's on every prior whose two costs differ at all, in both modes."""
    from oracle import ro
    from revo_amd import api
    _clear(monkeypatch)
    lvl = fc.SB.pyr_min_lvl
    poses = [fc.shift_pose(lvl, *k) for k in fc.SHIFTS + tuple(fc.RIM_RULES.values())]
    o_ref, o_cur = fc.oracle_pyramids("B")
    ot = ro.Tracker(fc.SB, OS, TrackerSettings())
    L = ro.lib()
    L.ro_set_accum_double(1)
    try:
        c_eye = ot.eval_cost(np.eye(3), np.zeros(3), lvl, o_cur, o_ref)
        costs = [ot.eval_cost(R, T, lvl, o_cur, o_ref) for R, T in poses]
        want = [ot.trackFrames(o_ref, o_cur, R, T)["flags"] & 1 for R, T in poses]
    finally:
        L.ro_set_accum_double(0)
    assert want == [int(c_eye < c) for c in costs] and 0 < sum(want) < len(want), (want, c_eye, costs)
    for exact in (True, False):
        cam = api.CameraPyr(fc.SB, exact_sums=exact)
        api.TrackerNew(TrackerSettings(check_init_values=1), fc.SB, cam)
        bt, keep = _batch(cam, "B", len(poses))
        got = [r["flags"] for r in _records(_track(bt, poses))]
        assert [g for g, c in zip(got, costs) if c != c_eye] == [w for w, c in zip(want, costs) if c != c_eye], (exact, got, want)


@pytest.mark.parametrize("scene", ["A", "B"])
def test_batch_pair_info_one_pose_per_pair(monkeypatch, scene):
    """e. revo_batch_pair_info with host poses, one launch per level and one case per pair: every record is the bytes of the
    single call."""
    _clear(monkeypatch)
    cam = _dev(scene, False)[0]
    single = _single_infos(scene)
    per_level = [[c for c in fc.cases(scene) if c[1] == lvl] for lvl in range(fc.NLEVELS)]
    bt, keep = _batch(cam, scene, len(per_level[0]))
    for lvl, cs in enumerate(per_level):
        RT = np.stack([np.concatenate([np.asarray(R, np.float32).T.reshape(9), np.asarray(T, np.float32)]) for _, _, R, T in cs])
        got = bt.pair_info(RT=RT, lvl=lvl)
        assert len(got) == len(cs)
        diff = [name for (name, _, _, _), g in zip(cs, got) if bytes(g) != single[(name, lvl)]]
        assert not diff, (scene, lvl, diff)


def test_quality_vote_with_far_poses_in_the_past_list(monkeypatch):
    """f. test_assess_tracking_quality_parity's pattern at 160x120 with a half turn and the through pose among the stored
    clouds' poses: the histograms, the overlaps and the verdict are the oracle's after every addition."""
    from oracle import ro
    from revo_amd import api
    _clear(monkeypatch)
    p = fc.pair_a()
    o_ref, o_cur = fc.oracle_pyramids("A")

    def mat(name):
        M = np.eye(4)
        M[:3, :3], M[:3, 3] = fc.poses_a()[name]
        return M

    # the vote reads the first n_frames_hist_voting = 3 stored clouds: the far poses come first
    orders = [[mat("yaw180"), mat("through"), np.eye(4)], [p["T_ref_curr"], mat("through"), mat("yaw180")],
              [mat("behind"), synth.se3_exp([0.3, 0, 0, 0, 0.2, 0]), mat("yaw90")]]
    n_seen = 0
    for poses in orders:
        cam = api.CameraPyr(fc.SA)
        gt = api.TrackerNew(TrackerSettings(), fc.SA, cam)
        g_ref, g_cur = _frames(cam, "A")
        ot = ro.Tracker(fc.SA, OS, TrackerSettings())
        for k, P in enumerate(poses):
            src_g, src_o = (g_ref, o_ref) if k % 2 == 0 else (g_cur, o_cur)
            gt.addOldPclAndPose(src_g, 2, P, float(k))
            ot.addOldPclAndPose(src_o, 2, P, float(k))
            for est in (p["T_ref_curr"], mat("yaw180"), mat("through")):
                st_g, h_g, o_g = gt.assessTrackingQuality(est, g_cur, return_hist=True)
                st_o, h_o, o_o = ot.assessTrackingQuality(est, o_cur)
                assert np.array_equal(h_g, h_o) and np.array_equal(o_g, o_o) and st_g == st_o, (k, h_g, h_o, o_g, o_o, st_g, st_o)
                n_seen += int(h_o.sum() > 0)
        assert gt.pastSize() == ot.past_size() == 3
    assert n_seen >= 9  # the far clouds do land in the histogram
