"""k_track's LM ladder, Huber weight and edge-distance filter away from the default OptimizerSettings, on the MI355X, over the
matrix of tests/lm_settings_cases.py (16 seeded pairs at 160x120 and a reduced set at 320x240, from identity and from a prior).

a. Exact-sums mode: the records are the plain ladder's (one workgroup, one candidate per pass) byte for byte, whatever the
   cluster, the speculation depth, the batch size or the path.
b. Default mode: the speculation depth alone changes nothing.
c. The sequence lengths that the settings force, and under gn1 the counts of the evaluation the record reports.
d. Every case against the oracle with double sums, held to four times the reference's own float-against-double distance.
e. The per-point weights and the filter: evalAt and revo_tracker_pair_info against their numpy specifications, bit for bit.
f. checkInitializationValues under a tight filter."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import exact_sums_ref as xr  # noqa: E402
import lm_settings_cases as lc  # noqa: E402
import pair_info_ref as pr  # noqa: E402

KNOBS = ("REVO_TRACK_CLUSTER", "REVO_TRACK_CLUSTER_ONE", "REVO_TRACK_REDUNDANT_BATCH", "REVO_TRACK_REDUNDANT_ONE",
         "REVO_TRACK_KSPEC", "REVO_TRACK_KSPEC_ONE")
REC = 96  # sizeof(revo_pair_result)
MODES = [pytest.param(True, id="exact"), pytest.param(False, id="float")]


def _clear(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _set(cam, size, case, start, check_init=None, use_edge_filter=1):
    """The case's settings into the context (revo_ctx_set_tracker) -> the TrackerNew"""
    from revo_amd import api
    ts = lc.tracker_settings(start, check_init)
    ts.optimizerSettings = lc.optimizer_settings(case, use_edge_filter)
    return api.TrackerNew(ts, lc.SIZES[size], cam)


def _pyramids(cam, size, pairs):
    from revo_amd import api
    out = []
    for p in pairs:
        ref = api.ImgPyramidRGBD(lc.SIZES[size], cam, *p["ref"])
        cur = api.ImgPyramidRGBD(lc.SIZES[size], cam, *p["curr"])
        ref.makeKeyframe()
        out.append((ref, cur))
    return out


def _single(trk, pyrs, start):
    """the single-pair call on every pair -> per pair (R, T, err bytes, good, bad, status, evals)"""
    R0, T0 = lc.start_pose(start)
    out = []
    for ref, cur in pyrs:
        status, R, T, err = trk.trackFrames(R0, T0, ref, cur)
        info = trk.last_info
        out.append((np.asarray(R, np.float32).tobytes(), np.asarray(T, np.float32).tobytes(), np.float32(err).tobytes(),
                    info.good_pts_edges, info.bad_pts_edges, status, tuple(trk.last_evals.tolist())))
    return out


def _key(r):
    return (r["R"].tobytes(), r["T"].tobytes(), np.float32(r["err"]).tobytes(), r["good"], r["bad"], r["status"],
            tuple(r["evals"].tolist()))


class _Batches:
    """The 16 pairs resident in batches of n (built once); run(start) tracks them under the context's current settings
    from the start pose (the batch's init_RT interface) -> the 16 raw records."""

    def __init__(self, cam, pairs, n):
        import torch
        from revo_amd import api
        self.n, self.parts = n, []
        for b0 in range(0, len(pairs), n):
            part = pairs[b0:b0 + n]
            bgr = torch.from_numpy(np.stack([p[k][0] for p in part for k in ("ref", "curr")])).cuda()
            dep = torch.from_numpy(np.stack([p[k][1] for p in part for k in ("ref", "curr")])).cuda()
            bt = api.BatchTracker(cam, n)
            bt.build(bgr.data_ptr(), dep.data_ptr())
            bt.sync()
            self.parts.append((bt, bgr, dep))

    def run(self, start):
        """start: a start of lm_settings_cases for every pair, or one (R, T) per pair"""
        import torch
        from revo_amd import api
        poses = [lc.start_pose(start)] * (self.n * len(self.parts)) if isinstance(start, str) else list(start)
        out = []
        for k, (bt, _, _) in enumerate(self.parts):
            part = poses[k * self.n:(k + 1) * self.n]
            init = None if start == "id" else api.pack_init_RT([R for R, _ in part], [T for _, T in part])
            d_res = torch.zeros(self.n * REC, dtype=torch.uint8, device="cuda")
            bt.track_only(d_res.data_ptr(), init_RT=init)
            bt.sync()
            buf = d_res.cpu().numpy().tobytes()
            out += [buf[i * REC:(i + 1) * REC] for i in range(self.n)]
        return out


def _records(raw):
    from revo_amd import api
    return api.results_from_buffer(b"".join(raw), len(raw))


PARTITIONS = [  # (label, environment knobs, path); the first is the base: the plain, unspeculated ladder in one workgroup
    ("single-c1-red0-k1", {"REVO_TRACK_CLUSTER_ONE": "1", "REVO_TRACK_REDUNDANT_ONE": "0", "REVO_TRACK_KSPEC": "1"}, ("single", 1)),
    ("single-k2", {"REVO_TRACK_KSPEC_ONE": "2"}, ("single", 1)),
    ("single-k3", {"REVO_TRACK_KSPEC_ONE": "3"}, ("single", 1)),
    ("single-k4", {"REVO_TRACK_KSPEC_ONE": "4"}, ("single", 1)),
    ("single-c16", {"REVO_TRACK_CLUSTER_ONE": "16"}, ("single", 1)),
    ("batch16", {}, ("batch", 16)),
    ("batch16-c1", {"REVO_TRACK_CLUSTER": "1"}, ("batch", 16)),
    ("batch16-k4", {"REVO_TRACK_KSPEC": "4"}, ("batch", 16)),
    ("batch8-c8-red0", {"REVO_TRACK_CLUSTER": "8", "REVO_TRACK_REDUNDANT_BATCH": "0"}, ("batch", 8)),
]


@pytest.mark.parametrize("size", ["160", "320"])
def test_exact_records_are_the_plain_ladders_in_every_partition(monkeypatch, size):
    """Every case (`free` included, which runs into the noise) from both starts: in exact-sums mode the 16 records -- R, T, err,
    good / bad, status, evals; the whole 96 bytes among the batches -- are those of the single-pair call with one workgroup,
    no redundant evaluation and one candidate per pass, in every partition of PARTITIONS.  A fresh context per partition; the
    prior reaches the batches through revo_batch_track_only's init_RT.  No record carries flag 2, 4 or 8."""
    from revo_amd import api
    pairs = lc.pairs(size)
    cases = lc.matrix(size)
    base_keys, base_raw = {}, {}
    bad = []
    for label, env, (path, n) in PARTITIONS:
        _clear(monkeypatch)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        cam = api.CameraPyr(lc.SIZES[size], exact_sums=True)
        assert cam.exact_sums
        work = _pyramids(cam, size, pairs) if path == "single" else _Batches(cam, pairs, n)
        for case, start in cases:
            trk = _set(cam, size, case, start)
            if path == "single":
                keys = _single(trk, work, start)
            else:
                raw = work.run(start)
                recs = _records(raw)
                keys = [_key(r) for r in recs]
                flags = [r["flags"] for r in recs]
                if any(f & (2 | 4 | 8) for f in flags):
                    bad.append((label, case, start, "flags", flags))
                diff = [i for i in range(lc.NPAIRS) if raw[i] != base_raw.setdefault((case, start), raw)[i]]
                if diff:
                    bad.append((label, case, start, "records", diff))
            diff = [i for i in range(lc.NPAIRS) if keys[i] != base_keys.setdefault((case, start), keys)[i]]
            if diff:
                bad.append((label, case, start, "keys", diff, [(keys[i][6], base_keys[(case, start)][i][6]) for i in diff]))
        del work, trk, cam
    assert not bad, bad
    assert len(base_keys) == len(cases) and len(base_raw) == len(cases)


@pytest.mark.parametrize("size", ["160", "320"])
def test_speculation_depth_alone_changes_nothing_in_the_default_mode(monkeypatch, size):
    """The float path, the single-pair call on four workgroups: 1, 2 and 4 candidates per pass give the same pose, error,
    counts and evaluations for every case -- test_speculation_depth_and_cluster_shape_leave_the_lm_sequence_untouched over the matrix."""
    from revo_amd import api
    pairs = lc.pairs(size)
    base = {}
    bad = []
    for k in ("1", "2", "4"):
        _clear(monkeypatch)
        monkeypatch.setenv("REVO_TRACK_CLUSTER_ONE", "4")
        monkeypatch.setenv("REVO_TRACK_KSPEC", k)
        cam = api.CameraPyr(lc.SIZES[size])
        assert not cam.exact_sums
        pyrs = _pyramids(cam, size, pairs)
        for case, start in lc.matrix(size):
            keys = _single(_set(cam, size, case, start), pyrs, start)
            diff = [i for i in range(lc.NPAIRS) if keys[i] != base.setdefault((case, start), keys)[i]]
            if diff:
                bad.append((k, case, start, diff))
        del pyrs, cam
    assert not bad, bad
    assert sum(sum(key[6]) for keys in base.values() for key in keys) > 12 * lc.NPAIRS * len(base)


@functools.lru_cache(maxsize=None)
def _device_runs(size, exact):
    """Under the shipped knobs (the caller has cleared them): {(case, start): (single-pair keys, batch-of-16 records)}.
    Computed once per size and mode; do not modify."""
    from revo_amd import api
    pairs = lc.pairs(size)
    cam = api.CameraPyr(lc.SIZES[size], exact_sums=exact)
    pyrs = _pyramids(cam, size, pairs)
    batch = _Batches(cam, pairs, 16)
    out = {}
    for case, start in lc.matrix(size):
        trk = _set(cam, size, case, start)
        out[(case, start)] = (_single(trk, pyrs, start), _records(batch.run(start)))
    return out


@pytest.mark.parametrize("exact", MODES)
@pytest.mark.parametrize("size", ["160", "320"])
def test_forced_lengths_on_the_device(monkeypatch, size, exact):
    """gn1, cap3_nostep, caps123+smin: the lengths lm_settings_cases.check_forced_lengths states hold for last_evals and for the
    batch records; under gn1 the evals are the oracle's on every pair, and in exact mode so are good / bad -- there the
    last evaluation of a level is a rejected candidate on many pairs, which pins the evaluation the record reports."""
    _clear(monkeypatch)
    runs = _device_runs(size, exact)
    n_last_rejected = 0
    for (case, start), (single, batch) in runs.items():
        if case not in lc.FORCED:
            continue
        oracle = lc.oracle_runs(size, case, start, True)
        for i in range(lc.NPAIRS):
            for evals, good, bad in ((single[i][6], single[i][3], single[i][4]),
                                     (tuple(batch[i]["evals"].tolist()), batch[i]["good"], batch[i]["bad"])):
                where = (case, start, i, evals)
                lc.check_forced_lengths(case, evals)
                assert all(e == 0 for e in evals[3:]), where
                if case == "gn1":
                    assert tuple(evals[:3]) == oracle[i]["evals"], where
                    if exact:
                        assert (good, bad) == (oracle[i]["good"], oracle[i]["bad"]), where
            assert batch[i]["flags"] & (2 | 4 | 8) == 0
            if case == "gn1":
                n_last_rejected += oracle[i]["trace"][0] == (0,)
    if size == "160":
        assert n_last_rejected >= 1  # the record's counts (level 0's) are a rejected candidate's on some pair


@pytest.mark.parametrize("exact", MODES)
@pytest.mark.parametrize("size", ["160", "320"])
def test_against_the_double_sum_oracle(monkeypatch, capsys, size, exact):
    """Every case but `free`, the batch of 16 under the shipped knobs against the oracle with double sums.  Per case and start:
    at most 2 of the 16 pairs may differ from the oracle in their evals (the reference's float and double sums differ on at
    most 1); those are only held to a finite pose, clean flags and an error not above the one at the start pose.  On every
    other pair the pose lies within tol = max(1e-6, 4 d_self) of the oracle's, d_self being the oracle's own
    float-against-double distance under the case on the same pairs (the device's float sums sit no further from the
    double oracle than the oracle's float sums do; the factor leaves room for the other summation order and an ulp in the
    candidate pose); in exact mode good / bad are equal and err agrees to 1e-5 relative."""
    from oracle import ro
    _clear(monkeypatch)
    runs = _device_runs(size, exact)
    s = lc.SIZES[size]
    L = ro.lib()
    lines, bad = [], []
    for (case, start), (_, batch) in runs.items():
        if case == "free":
            continue
        oracle = lc.oracle_runs(size, case, start, True)
        _, d_self = lc.self_distance(size, case, start)
        tol = max(1e-6, 4.0 * d_self)
        same = [i for i in range(lc.NPAIRS) if tuple(batch[i]["evals"][:3].tolist()) == oracle[i]["evals"]]
        worst = 0.0
        if len(same) < lc.NPAIRS - 2:
            bad.append((case, start, "evals differ on", lc.NPAIRS - len(same)))
        R0, T0 = lc.start_pose(start)
        for i in range(lc.NPAIRS):
            r, o = batch[i], oracle[i]
            if r["flags"] & (2 | 4 | 8):
                bad.append((case, start, i, "flags", r["flags"]))
            if i in same:
                d = lc.pose_distance(r["R"], r["T"], o["R"], o["T"])
                worst = max(worst, d)
                if not d <= tol:
                    bad.append((case, start, i, "pose", d, tol))
                if exact and (r["good"], r["bad"]) != (o["good"], o["bad"]):
                    bad.append((case, start, i, "counts", (r["good"], r["bad"]), (o["good"], o["bad"])))
                if exact and not abs(r["err"] - o["err"]) <= 1e-5 * abs(o["err"]):
                    bad.append((case, start, i, "err", r["err"], o["err"]))
            else:
                L.ro_set_accum_double(1)
                try:
                    o_ref, o_cur = lc.oracle_pyramids(size)[i]
                    e0 = ro.Tracker(s, lc.optimizer_settings(case), lc.tracker_settings(start)).eval(o_ref, o_cur, R0, T0, 0)[0]
                finally:
                    L.ro_set_accum_double(0)
                if not (np.all(np.isfinite(r["R"])) and np.all(np.isfinite(r["T"])) and r["err"] <= e0):
                    bad.append((case, start, i, "differing pair", r["err"], e0))
        lines.append("| %s | %s | %s | %s | %d/16 | %.2e | %.2e | %.2e |" % (size, "exact" if exact else "float", case, start, len(same), worst,
                                                                          d_self, tol))
    with capsys.disabled():
        print("\n| size | sums | case | start | equal evals | largest distance | d_self | tol |\n" + "\n".join(lines))
    assert not bad, bad


def _cam6(cam, lvl):
    c = cam.at(lvl)
    return (c.fx, c.fy, c.cx, c.cy, c.width, c.height)


def test_weights_and_filter_bit_for_bit(monkeypatch):
    """Exact mode, two 320x240 pairs, three levels, at the identity, half the true translation and the tracked pose, under each
    Huber threshold and edge distance of lm_settings_cases.WEIGHT_CASES with the filter on and off (the settings go in through
    TrackerNew / revo_ctx_set_tracker): Optimizer.evalAt is exact_sums_ref.exact_eval -- A, b, err, sum_error_weighted,
    sum_error_unweighted, the counts -- and revo_tracker_pair_info is pair_info_ref.pair_info, bit for bit.  That the setting
    arrived shows against the default's sums at the same pose: see test_optimizer_settings_cpu.py for what can differ."""
    from revo_amd import api
    _clear(monkeypatch)
    size, s = "320", lc.S320
    cam = api.CameraPyr(s, exact_sums=True)
    pyrs = _pyramids(cam, size, lc.pairs(size)[:2])
    trk = _set(cam, size, None, "id")
    poses = []
    for p, (ref, cur) in zip(lc.pairs(size), pyrs):
        _, Rc, Tc, _ = trk.trackFrames(np.eye(3), np.zeros(3), ref, cur)
        gt = p["T_ref_curr"]
        poses.append([(np.eye(3), np.zeros(3)), (gt[:3, :3], 0.5 * gt[:3, 3]), (Rc, Tc)])
    dflt = {}
    n_eval = n_fewer = 0
    for name in (None,) + tuple(lc.WEIGHT_CASES):
        for filt in (1, 0):
            os_ = lc.optimizer_settings(name, filt)
            trk = _set(cam, size, name, "id", use_edge_filter=filt)
            opt = api.Optimizer(os_, cam)
            for pi, (ref, cur) in enumerate(pyrs):
                for lvl in range(s.nLevels()):
                    args = (ref.returnOptimizationStructure(lvl), cur.return3DEdges(lvl), _cam6(cam, lvl))
                    tail = (os_.edge_distance_lvl[lvl], os_.use_edge_filter, os_.huber_edge)
                    for qi, (R, T) in enumerate(poses[pi]):
                        where = (name, filt, pi, lvl, qi)
                        err, info, A, b = opt.evalAt(ref, cur, R, T, lvl)
                        e_x, sw, su, good, bad, A_x, b_x = xr.exact_eval(*args, R, T, *tail)
                        assert (info.good_pts_edges, info.bad_pts_edges) == (good, bad), where
                        assert np.float32(info.sum_error_weighted).tobytes() == sw.tobytes(), where
                        assert np.float32(info.sum_error_unweighted).tobytes() == su.tobytes(), where
                        assert np.float32(err).tobytes() == e_x.tobytes(), where
                        assert np.asarray(A, np.float32).tobytes() == A_x.tobytes(), (where, A - A_x)
                        assert np.asarray(b, np.float32).tobytes() == b_x.tobytes(), (where, b - b_x)
                        assert bytes(trk.pairInfo(ref, cur, R, T, lvl)) == pr.pair_info(*args, R, T, *tail, level=lvl), where
                        n_eval += 1
                        at = (pi, lvl, qi)
                        if name is None:
                            dflt[(filt,) + at] = (good, sw.tobytes())
                        elif name.startswith("huber"):
                            assert good == dflt[(filt,) + at][0] and sw.tobytes() != dflt[(filt,) + at][1], where
                        elif filt and name == "edist322":
                            assert good <= dflt[(1,) + at][0], where
                            n_fewer += int(good < dflt[(1,) + at][0])
                        else:  # nothing is filtered: the sums of the filter switched off
                            assert (good, sw.tobytes()) == dflt[(0,) + at], where
    assert n_eval == (1 + len(lc.WEIGHT_CASES)) * 2 * 2 * 3 * 3
    assert n_fewer >= 9


@pytest.mark.parametrize("exact", MODES)
def test_one_gauss_newton_step_per_level_against_the_oracle(monkeypatch, exact):
    """gn1 through Optimizer.trackFrames level by level (two 320x240 pairs, from the identity and from half the true
    translation): the oracle's track_level takes 2 evaluations, and the device's pose is within max(1e-6, 4 d_self) of the
    double oracle's, d_self the oracle's float-against-double distance of the same call; in exact mode good / bad are equal --
    also where the one candidate was rejected, so that the counts are its and not the accepted pose's."""
    from oracle import ro
    from revo_amd import api
    _clear(monkeypatch)
    size, s = "320", lc.S320
    cam = api.CameraPyr(s, exact_sums=exact)
    pyrs = _pyramids(cam, size, lc.pairs(size)[:2])
    trk = _set(cam, size, "gn1", "id")
    ot = ro.Tracker(s, lc.optimizer_settings("gn1"), lc.tracker_settings("id"))
    L = ro.lib()
    trace = np.zeros(8, np.uint8)
    n = n_rejected = 0
    for p, (ref, cur), (o_ref, o_cur) in zip(lc.pairs(size), pyrs, lc.oracle_pyramids(size)):
        gt = p["T_ref_curr"]
        for R0, T0 in ((np.eye(3), np.zeros(3)), (gt[:3, :3], 0.5 * gt[:3, 3])):
            for lvl in range(s.nLevels()):
                Rf, Tf, _, _, ev_f, _ = ot.track_level(o_ref, o_cur, R0, T0, lvl)
                L.ro_set_accum_double(1)
                L.ro_lm_trace(1)
                try:
                    Rd, Td, err_d, info_d, ev_d, ab = ot.track_level(o_ref, o_cur, R0, T0, lvl)
                    assert L.ro_lm_trace_get(trace.ctypes.data_as(ro.u8p), len(trace)) == 1
                    n_rejected += int(trace[0] & 1) == 0
                finally:
                    L.ro_lm_trace(0)
                    L.ro_set_accum_double(0)
                assert (ev_f, ev_d, ab) == (2, 2, 0)
                tol = max(1e-6, 4.0 * lc.pose_distance(Rf, Tf, Rd, Td))
                info = api.ResidualInfo()
                err, R, T = trk.mOptimizer.trackFrames(ref, cur, R0, T0, lvl, info)
                d = lc.pose_distance(R, T, Rd, Td)
                print("gn1 level %d: device to double oracle %.3g, tol %.3g" % (lvl, d, tol))
                assert d <= tol, (lvl, d, tol)
                if exact:
                    assert (info.good_pts_edges, info.bad_pts_edges) == (info_d.good_pts_edges, info_d.bad_pts_edges), lvl
                n += 1
    assert n == 12
    assert n_rejected >= 3  # the counts compared are a rejected candidate's on a quarter of the calls or more


@pytest.mark.parametrize("exact", MODES)
def test_check_initialization_values_under_a_tight_filter(monkeypatch, exact):
    """edist322+smin with check_init_values on (160x120, the batch of 16): the filtered costs of the identity and of the start
    pose decide whether the tracker keeps the start.  Once from the prior on every pair (which loses to the identity everywhere),
    once from every pair's true motion (which the summed cost of the 40x30 level keeps on a few pairs only: both outcomes):
    flags & 1 is the oracle's on every pair whose two oracle costs (double sums) differ by more than 1e-5 relative, and at
    least 12 of the 16 pairs are such."""
    from oracle import ro
    from revo_amd import api
    _clear(monkeypatch)
    size, case = "160", "edist322+smin"
    s = lc.SIZES[size]
    cam = api.CameraPyr(s, exact_sums=exact)
    batch = _Batches(cam, lc.pairs(size), 16)
    _set(cam, size, case, "prior", check_init=1)
    ot = ro.Tracker(s, lc.optimizer_settings(case), lc.tracker_settings("prior", 1))
    prior = lc.start_pose("prior")
    mixed = [(p["T_ref_curr"][:3, :3].astype(np.float32), p["T_ref_curr"][:3, 3].astype(np.float32)) for p in lc.pairs(size)]
    L = ro.lib()
    for starts in ([prior] * lc.NPAIRS, mixed):
        recs = _records(batch.run(starts))
        decided, want = [], []
        L.ro_set_accum_double(1)
        try:
            for (o_ref, o_cur), (R0, T0) in zip(lc.oracle_pyramids(size), starts):
                c_eye = ot.eval_cost(np.eye(3), np.zeros(3), s.pyr_min_lvl, o_cur, o_ref)
                c_init = ot.eval_cost(R0, T0, s.pyr_min_lvl, o_cur, o_ref)
                want.append(ot.trackFrames(o_ref, o_cur, R0, T0)["flags"] & 1)
                assert want[-1] == int(c_eye < c_init)
                decided.append(abs(c_eye - c_init) > 1e-5 * max(c_eye, c_init))
        finally:
            L.ro_set_accum_double(0)
        assert sum(decided) >= 12, decided
        got = [r["flags"] & 1 for r in recs]
        print("check_init under edist322: reset to identity on %d of %d decided pairs" % (sum(w for w, d in zip(want, decided) if d), sum(decided)))
        assert [g for g, d in zip(got, decided) if d] == [w for w, d in zip(want, decided) if d], (got, want, decided)
        assert all(r["flags"] & (2 | 4 | 8) == 0 for r in recs)
        if starts is mixed:
            assert 1 <= sum(w for w, d in zip(want, decided) if d) <= sum(decided) - 1, want  # both outcomes occur
