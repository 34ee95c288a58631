"""k_track and k_pair_info at every limit of their work split, on the MI355X, over the table of tests/track_split_cases.py
(tests/test_track_split_cpu.py proves that every case has the point counts and takes the paths the table states).

a. Exact-sums mode, evaluation: Optimizer.evalAt is exact_sums_ref.exact_eval and TrackerNew.pairInfo is pair_info_ref.pair_info,
   bit for bit, for every case at both poses under every single-pair partition (cluster 1, 2, 4, 16, 32; threshold 0 or shipped;
   1-4 candidates per pass).
b. Exact-sums mode, tracking: from the prior every case's key (R, T, err, good, bad, status, evals) is the plain ladder's in every
   partition; the batches of 13 and of 4 give the single-pair keys of the same pairs and equal records among themselves; no
   record carries flag 2, 4 or 8.
c. Default (float) mode: the speculation depth alone changes nothing at the limits; good = N and bad = 0 exactly in every
   partition; every sum within (N + 8) 2^-24 sum|t_i| of the exact sum; a redundant level gives one workgroup's bits.
d. checkInitializationValues (the MODE_COST pass): flags & 1 is the specification's in both modes under every cluster.
e. Empty levels, level by level.

A fresh context per partition (the knobs are read when a context or a batch is created).  The specifications are computed
once per case and shared; they are not modified."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from revo_amd.settings import OptimizerSettings, TrackerSettings, PLANE_DT, PLANE_EDGES3D, PLANE_GRADTABLE  # noqa: E402

import exact_sums_ref as xr  # noqa: E402
import pair_info_ref as pr  # noqa: E402
import track_split_cases as tc  # noqa: E402

KNOBS = ("REVO_TRACK_CLUSTER", "REVO_TRACK_CLUSTER_ONE", "REVO_TRACK_REDUNDANT_BATCH", "REVO_TRACK_REDUNDANT_ONE",
         "REVO_TRACK_KSPEC", "REVO_TRACK_KSPEC_ONE")
REC = 96  # sizeof(revo_pair_result)
OS = OptimizerSettings()
MODES = [pytest.param(True, id="exact"), pytest.param(False, id="float")]
IU = np.triu_indices(6)

TRACKED = tc.cases_of(range(1, 7))            # rows 1-6: one level, tracked and evaluated
INFO_ONLY = [n for n in tc.cases_of((10,)) if n not in TRACKED]
DECIDERS = tc.cases_of((4,), decider=True)
PYR = tc.pyr_cases()
ROW7 = [n for n in PYR if 7 in tc.CASES[n]["rows"]]
ROW8 = [n for n in PYR if 8 in tc.CASES[n]["rows"]]
SIZES = ("160", "320", "640", "640t", "pyr")


def _env(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _cam6(cam, lvl):
    c = cam.at(lvl)
    return (c.fx, c.fy, c.cx, c.cy, c.width, c.height)


def _case(name):
    return tc.CASES[name] if isinstance(name, str) else name


class _Ctx:
    """One context of a size under the knobs that are set now: the keyframe once, the current frames as they are asked for."""

    def __init__(self, size, exact, check_init=0):
        from revo_amd import api
        self.api, self.size, self.s = api, size, tc.settings_of(size)
        self.cam = api.CameraPyr(self.s, exact_sums=exact)
        assert bool(self.cam.exact_sums) == exact
        self.trk = api.TrackerNew(TrackerSettings(check_init_values=check_init), self.s, self.cam)
        self.opt = api.Optimizer(OS, self.cam)
        self._ref = None

    def pyrs(self, case):
        case = _case(case)
        ref, cur = tc.frames_of(case)
        if self._ref is None or case["size"] == "pyr":
            self._ref = self.api.ImgPyramidRGBD(self.s, self.cam, *ref)
            self._ref.makeKeyframe()
        return self._ref, self.api.ImgPyramidRGBD(self.s, self.cam, *cur)

    def key(self, ref, cur, R, T):
        status, Ro, To, err = self.trk.trackFrames(R, T, ref, cur)
        info = self.trk.last_info
        return (np.asarray(Ro, np.float32).tobytes(), np.asarray(To, np.float32).tobytes(), np.float32(err).tobytes(),
                info.good_pts_edges, info.bad_pts_edges, status, tuple(self.trk.last_evals.tolist()))


def _key(r):
    return (r["R"].tobytes(), r["T"].tobytes(), np.float32(r["err"]).tobytes(), r["good"], r["bad"], r["status"], tuple(r["evals"].tolist()))


def _oracle(name):
    """(settings, the oracle's keyframe, its current frame) of a case of CASES, or of ("batch", size, N): built when asked for
    and not kept (what is kept are the specifications made from them)."""
    from oracle import ro
    c = tc.CASES[name] if isinstance(name, str) else tc.batch_case(*name[1:])
    s = tc.settings_of(c["size"])
    ref, cur = tc.frames_of(c)
    o_ref, o_cur = ro.Pyramid(s, *ref), ro.Pyramid(s, *cur)
    o_ref.makeKeyframe()
    return s, o_ref, o_cur


@functools.lru_cache(maxsize=None)
def _spec(name, lvl, pose):
    """The specification of a case at a level and a pose (0: identity, 1: the size's prior): exact_eval's tuple, the pair-info
    record, and per sum (27 normal equations, sum w r^2, sum r^2) the exact sum and sum|t_i| in float64.  Do not modify."""
    s, o_ref, o_cur = _oracle(name)
    R, T = tc.poses_of(tc.CASES[name])[pose]
    cam = tuple(float(x) for x in o_cur.camera(lvl)[:4]) + (s.width >> lvl, s.height >> lvl)
    args = (o_ref.read(PLANE_GRADTABLE, lvl), o_cur.read(PLANE_EDGES3D, lvl), cam, R, T, OS.edge_distance_lvl[lvl], OS.use_edge_filter, OS.huber_edge)
    terms, sw, su, good, bad = xr.point_terms(*args)
    t64 = np.concatenate([terms, sw[None], su[None]]).astype(np.float64)
    return dict(eval=xr.exact_eval(*args), info=pr.pair_info(*args, level=lvl), sums=t64.sum(axis=1), abs=np.abs(t64).sum(axis=1),
                good=good, bad=bad, cam=cam)


def _levels(name):
    return range(len(tc.CASES[name]["levels"]))


def _same_bits(a, b):
    """equal bytes; a NaN equals a NaN (0 / 0 comes with either sign)"""
    a, b = np.atleast_1d(np.asarray(a, np.float32)), np.atleast_1d(np.asarray(b, np.float32))
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and a[~nan].tobytes() == b[~nan].tobytes()


def _check_exact_eval(ctx, name, ref, cur, where, info_too=True):
    n = 0
    for lvl in _levels(name):
        for pose, (R, T) in enumerate(tc.poses_of(tc.CASES[name])):
            sp = _spec(name, lvl, pose)
            at = where + (name, lvl, pose)
            assert np.array_equal(np.float32(sp["cam"]), np.float32(_cam6(ctx.cam, lvl))), at
            err, info, A, b = ctx.opt.evalAt(ref, cur, R, T, lvl)
            e_x, sw, su, good, bad, A_x, b_x = sp["eval"]
            assert (info.good_pts_edges, info.bad_pts_edges) == (good, bad), at
            assert np.float32(info.sum_error_weighted).tobytes() == sw.tobytes(), at
            assert np.float32(info.sum_error_unweighted).tobytes() == su.tobytes(), at
            assert _same_bits(err, e_x), at
            assert _same_bits(A, A_x), (at, A - A_x)
            assert _same_bits(b, b_x), (at, b - b_x)
            if info_too:
                assert bytes(ctx.trk.pairInfo(ref, cur, R, T, lvl)) == sp["info"], at
            n += 1
    return n


@pytest.mark.parametrize("part", tc.SINGLE, ids=[p[0] for p in tc.SINGLE])
def test_exact_evaluation_is_the_specification_at_every_limit(monkeypatch, part):
    """a. Every case of rows 1-7 at the identity and at the prior (the three-level cases at each level): A, b, err,
    sum_error_weighted, sum_error_unweighted, good and bad of evalAt are exact_eval's and the 192 bytes of pairInfo are
    pair_info's.  The cases of row 10 go through pairInfo (and evalAt) in the base partition and under the largest cluster."""
    label, env, C, r, k = part
    _env(monkeypatch, env)
    n = 0
    for size in SIZES:
        ctx = _Ctx(size, True)
        names = [x for x in TRACKED + ROW7 + (INFO_ONLY if C in (1, 32) and r == 0 else []) if tc.CASES[x]["size"] == size]
        for name in names:
            ref, cur = ctx.pyrs(name)
            if part is tc.SINGLE[0]:
                assert tuple(cur.return3DEdges(l).shape[0] for l in _levels(name)) == tc.CASES[name]["levels"], name
            n += _check_exact_eval(ctx, name, ref, cur, (label,))
        del ctx
    assert n >= 2 * len(TRACKED) + 6 * len(ROW7)


def _oracle_trace(name):
    """(evals, the accept / reject bits) of the oracle's trackFrames of a case from the prior, float sums"""
    from oracle import ro
    s, o_ref, o_cur = _oracle(name)
    L = ro.lib()
    buf = np.zeros(4096, np.uint8)
    ot = ro.Tracker(s, OS, TrackerSettings(check_init_values=0))
    L.ro_lm_trace(1)
    try:
        r = ot.trackFrames(o_ref, o_cur, *tc.prior_of(tc.CASES[name]["size"]))
        n = L.ro_lm_trace_get(buf.ctypes.data_as(ro.u8p), len(buf))
    finally:
        L.ro_lm_trace(0)
    return tuple(int(x) for x in r["evals"][:s.nLevels()]), (buf[:n] & 1).tolist()


def _run_batch(ctx, size, Ns, start):
    """One batch of the size's noise image with Ns points per pair, tracked from `start` -> (raw records, the batch)"""
    import torch
    frames = [tc.frames_of(tc.batch_case(size, N)) for N in Ns]
    bgr = torch.from_numpy(np.stack([f[k][0] for f in frames for k in (0, 1)])).cuda()
    dep = torch.from_numpy(np.stack([f[k][1] for f in frames for k in (0, 1)])).cuda()
    bt = ctx.api.BatchTracker(ctx.cam, len(Ns))
    bt.build(bgr.data_ptr(), dep.data_ptr())
    d_res = torch.zeros(len(Ns) * REC, dtype=torch.uint8, device="cuda")
    bt.track_only(d_res.data_ptr(), init_RT=ctx.api.pack_init_RT([start[0]] * len(Ns), [start[1]] * len(Ns)))
    bt.sync()
    buf = d_res.cpu().numpy().tobytes()
    return [buf[i * REC:(i + 1) * REC] for i in range(len(Ns))]


def test_exact_tracking_is_the_plain_ladders_at_every_limit(monkeypatch):
    """b. From the prior: the key of every case of rows 1-6 under every single-pair partition, and of every three-level case
    (rows 7, 8; also from the identity) under its own threshold with 4 and 16 workgroups, is the base partition's (one
    workgroup, one candidate per pass).  Row 9: the batch of 13 (640 x 240, cluster 1, 2, 4, 8) and the batch of 4 (640 x 288,
    cluster 32) give the single-pair keys of the same pairs, the whole 96 bytes agree among the batch partitions, and no
    record carries flag 2, 4 or 8 (the single-pair call turns 2 and 8 into errors).  Tracking ran: the base keys hold at least
    three evaluations per case with 63 points and more, and on at least three cases whose evals are the oracle's the oracle
    rejected a candidate -- with 2-4 candidates per pass those rejections sit in fused_block's retry lanes."""
    bad = []
    base, seen = {}, 0
    for label, env, C, r, k in tc.SINGLE:
        _env(monkeypatch, env)
        for size in SIZES[:4]:
            ctx = _Ctx(size, True)
            names = [x for x in TRACKED if tc.CASES[x]["size"] == size]
            extra = [("batch", size, N) for N in {"640": tc.BATCH13, "640t": tc.BATCH4_N}.get(size, ())] if label == tc.SINGLE[0][0] else []
            for name in names + extra:
                ref, cur = ctx.pyrs(name if isinstance(name, str) else tc.batch_case(*name[1:]))
                key = ctx.key(ref, cur, *tc.prior_of(size))
                if key != base.setdefault(name, key):
                    bad.append((label, name, key[3:], base[name][3:]))
                seen += 1
            del ctx
    for name in PYR:
        for label, env, C, r, k in tc.pyr_partitions(tc.CASES[name]):
            _env(monkeypatch, env)
            ctx = _Ctx("pyr", True)
            ref, cur = ctx.pyrs(name)
            for start, pose in enumerate(tc.poses_of(tc.CASES[name])):
                key = ctx.key(ref, cur, *pose)
                if key != base.setdefault((name, start), key):
                    bad.append((label, name, start, key[3:], base[(name, start)][3:]))
            del ctx
    raws = {}
    for (label, env, C, r, k), size, Ns in [(p, "640", tc.BATCH13) for p in tc.BATCH] + [(tc.BATCH4, "640t", tc.BATCH4_N)]:
        _env(monkeypatch, env)
        ctx = _Ctx(size, True)
        raw = _run_batch(ctx, size, Ns, tc.prior_of(size))
        recs = ctx.api.results_from_buffer(b"".join(raw), len(raw))
        for i, N in enumerate(Ns):
            if recs[i]["flags"] & (2 | 4 | 8):
                bad.append((label, N, "flags", recs[i]["flags"]))
            if _key(recs[i]) != base[("batch", size, N)]:
                bad.append((label, N, "key", _key(recs[i])[3:], base[("batch", size, N)][3:]))
            if raw[i] != raws.setdefault((size, N), raw[i]):
                bad.append((label, N, "record"))
            if recs[i]["n_pts0"] != N:
                bad.append((label, N, "n_pts0", recs[i]["n_pts0"]))
        del ctx
    assert not bad, bad
    assert seen == len(tc.SINGLE) * len(TRACKED) + len(tc.BATCH13) + len(tc.BATCH4_N)
    assert all(sum(base[n][6]) >= 3 for n in TRACKED if tc.CASES[n]["N"] >= 63), {n: base[n][6] for n in TRACKED}
    with_reject = 0
    for name in TRACKED:
        evals, trace = _oracle_trace(name)
        with_reject += int(base[name][6][:len(evals)] == evals and 0 in trace)
    assert with_reject >= 3, with_reject


def test_float_keys_do_not_depend_on_the_speculation_depth(monkeypatch):
    """c. The default mode with four workgroups and the shipped threshold: 1, 2, 3 and 4 candidates per pass give the same key
    for every case of rows 1-8 from the prior -- the loops of full_point against those of fused_block<1..3> at the limits."""
    base, bad = {}, []
    for k in (1, 2, 3, 4):
        _env(monkeypatch, tc._one(4, tc.R_ONE, k)[1])
        for size in SIZES:
            ctx = _Ctx(size, False)
            for name in [x for x in TRACKED + PYR if tc.CASES[x]["size"] == size]:
                ref, cur = ctx.pyrs(name)
                key = ctx.key(ref, cur, *tc.poses_of(tc.CASES[name])[1])
                if key != base.setdefault(name, key):
                    bad.append((k, name, key[3:], base[name][3:]))
            del ctx
    assert not bad, bad
    assert all(sum(base[n][6]) >= 3 for n in TRACKED if tc.CASES[n]["N"] >= 63)


def test_float_counts_are_exact_and_sums_within_the_summation_bound(monkeypatch, capsys):
    """c. The default mode, every case of rows 1-6 at both poses under every single-pair partition: good = N and bad = 0 exactly
    (the sharp check at large N), and every sum -- A n, b n, sum_error_weighted, sum_error_unweighted -- within
    (N + 8) 2^-24 sum|t_i| of the exact sum, sum|t_i| from point_terms in float64 (the sharp check at small N): N - 1 roundings
    bound any summation order of N floats, 8 ulp per term cover the documented per-term differences of the float path (fmaf,
    z z); A, b and err are compared after the division by n, with one more ulp.  Where a partition evaluates a level
    redundantly, evalAt returns the bits of the one-workgroup partition (same threads, same order).  N = 0: the counts alone
    (the sums are 0 / 0)."""
    worst, bad, base = {}, [], {}
    eps = 2.0 ** -24
    for label, env, C, r, k in tc.SINGLE:
        _env(monkeypatch, env)
        for size in SIZES[:4]:
            ctx = _Ctx(size, False)
            for name in [x for x in TRACKED if tc.CASES[x]["size"] == size]:
                N = tc.CASES[name]["N"]
                ref, cur = ctx.pyrs(name)
                for pose, (R, T) in enumerate(tc.poses_of(tc.CASES[name])):
                    sp = _spec(name, 0, pose)
                    err, info, A, b = ctx.opt.evalAt(ref, cur, R, T, 0)
                    if (info.good_pts_edges, info.bad_pts_edges) != (N, 0):
                        bad.append((label, name, pose, "counts", info.good_pts_edges, info.bad_pts_edges))
                    bits = (np.float32(err).tobytes(), A.tobytes(), b.tobytes(), info.sum_error_weighted, info.sum_error_unweighted)
                    if C == 1:
                        base.setdefault((name, pose), bits)
                    elif tc.redundant(N, C, r) and N > 0 and bits != base[(name, pose)]:
                        bad.append((label, name, pose, "a redundant level differs from one workgroup's bits"))
                    if N == 0:
                        continue
                    tol = (N + 8) * eps * sp["abs"]
                    got = np.concatenate([np.asarray(A, np.float64)[IU], -np.asarray(b, np.float64), [err]])
                    want = np.concatenate([sp["sums"][:27], sp["sums"][27:28]]) / N
                    tol_n = np.concatenate([tol[:27], tol[27:28]]) / N + 2.0 * eps * np.abs(want)
                    d = np.concatenate([np.abs(got - want), np.abs(np.array([info.sum_error_weighted, info.sum_error_unweighted]) - sp["sums"][27:])])
                    t = np.concatenate([tol_n, tol[27:]])
                    ratio = float(np.max(np.where(t > 0, d / np.where(t > 0, t, 1.0), np.where(d > 0, np.inf, 0.0))))
                    for row in tc.CASES[name]["rows"]:
                        worst[row] = max(worst.get(row, 0.0), ratio)
                    if ratio > 1.0:
                        bad.append((label, name, pose, "sums", ratio))
            del ctx
    with capsys.disabled():
        print("\nfloat mode, largest |sum - exact| / bound per row: " + ", ".join("row %d: %.3f" % (row, worst[row]) for row in sorted(worst)))
    assert not bad, bad
    assert set(worst) >= set(range(1, 7))


def _cost_flag(name, prior):
    """flags & 1 of the specification: eval_cost(identity) < eval_cost(prior) at the coarsest level (the only one here)"""
    s, o_ref, o_cur = _oracle(name)
    dt, pts = o_ref.read(PLANE_DT, 0), o_cur.read(PLANE_EDGES3D, 0)
    cam = (s.fx, s.fy, s.cx, s.cy, s.width, s.height)
    cost = [xr.eval_cost(dt, pts, cam, R, T, OS.edge_distance_lvl[0], OS.use_edge_filter) for R, T in (tc.IDENTITY, prior)]
    return int(cost[0] < cost[1]), cost


@pytest.mark.parametrize("exact", MODES)
def test_the_init_check_decides_as_the_specification_at_every_limit(monkeypatch, exact):
    """d. check_init_values = 1, batches of one pair (their records carry the flags, which the single-pair call does not
    return) under 1, 2, 4, 16 and 32 workgroups with the threshold at 0 and shipped: for every case of rows 1-6 started from
    the prior, and for the deciders started from their shift prior, flags & 1 is eval_cost(identity) < eval_cost(prior) of
    exact_sums_ref; started from the identity the costs tie and the flag is 0.  The batch of 13 under its partitions likewise.
    The limit of this check: a point lost by the MODE_COST loop shows only where it decides the comparison.  Over the
    noise image the identity costs 0 at most points and the prior more, so the plain cases are decided by hundreds of
    points and would not notice one.  The deciders are built for it: all their points but one cost 0 under both poses, and
    the one that does not is the last of the tile-ordered list, the only point their level streams (the test checks that on
    the device's list) -- without it the flag is 0, with it 1."""
    import torch
    want_flags = {}
    bad, ones = [], 0
    for label, env, C, r, k in tc.COST:
        _env(monkeypatch, env)
        for size in SIZES[:4]:
            names = [x for x in TRACKED + DECIDERS if tc.CASES[x]["size"] == size]
            ctx = _Ctx(size, exact, check_init=1)
            bt = ctx.api.BatchTracker(ctx.cam, 1)
            d_res = torch.zeros(REC, dtype=torch.uint8, device="cuda")
            for name in names:
                c = tc.CASES[name]
                prior = tc.shift_prior(size) if c["special"] else tc.prior_of(size)
                if name not in want_flags:
                    want_flags[name] = _cost_flag(name, prior)[0]
                    if c["special"]:
                        ref, cur = ctx.pyrs(name)
                        assert cur.edges3DTiled(0)[-1, 2] == np.float32(tc.SPECIAL_DEPTH) and cur.edges3DTiled(0).shape[0] == c["N"], name
                ref, cur = tc.frames_of(c)
                bgr = torch.from_numpy(np.stack([ref[0], cur[0]])).cuda()
                dep = torch.from_numpy(np.stack([ref[1], cur[1]])).cuda()
                bt.build(bgr.data_ptr(), dep.data_ptr())
                for start, want in ((prior, want_flags[name]), (tc.IDENTITY, 0)):
                    bt.track_only(d_res.data_ptr(), init_RT=ctx.api.pack_init_RT([start[0]], [start[1]]))
                    bt.sync()
                    rec = ctx.api.results_from_buffer(d_res.cpu().numpy().tobytes(), 1)[0]
                    if rec["flags"] != want:
                        bad.append((label, name, "identity" if start is tc.IDENTITY else "prior", rec["flags"], want))
                    ones += want
            del bt, ctx
    for label, env, C, r, k in tc.BATCH:  # row 9: the 13 pairs decide independently in one grid
        _env(monkeypatch, env)
        ctx = _Ctx("640", exact, check_init=1)
        prior = tc.prior_of("640")
        recs = ctx.api.results_from_buffer(b"".join(_run_batch(ctx, "640", tc.BATCH13, prior)), len(tc.BATCH13))
        want = [want_flags.setdefault(("batch", "640", N), _cost_flag(("batch", "640", N), prior)[0]) for N in tc.BATCH13]
        if [rec["flags"] for rec in recs] != want:
            bad.append((label, [rec["flags"] for rec in recs], want))
        del ctx
    assert not bad, bad
    assert 1 <= sum(want_flags[("batch", "640", N)] for N in tc.BATCH13) <= 12  # both outcomes in one grid
    assert all(want_flags[n] == 1 for n in DECIDERS) and ones >= len(tc.COST) * len(DECIDERS)
    assert 5 <= sum(want_flags[n] for n in TRACKED) <= len(TRACKED) - 5, want_flags  # both outcomes among the plain cases (the small ones tie)


@pytest.mark.parametrize("exact", MODES)
def test_empty_levels_level_by_level(monkeypatch, exact):
    """e. Row 8 through Optimizer.trackFrames on the empty level, under the case's partitions, from the identity and from the
    prior: err is NaN, good = bad = 0, T comes back bit for bit and R as the oracle's track_level returns it (the identity bit
    for bit; a rotation passes through the quaternion of Sophus::SE3f, in the reference as here).  The level call does not
    return its evaluation count: the full trackFrames of the case reports it per level, and there the empty level's count is
    the oracle's track_level count.  (The full trackFrames of these cases is held to the plain ladder's by test b.)"""
    from oracle import ro
    n = 0
    for name in ROW8:
        c = tc.CASES[name]
        lvl = c["levels"].index(0)
        s, o_ref, o_cur = _oracle(name)
        ot = ro.Tracker(s, OS, TrackerSettings(check_init_values=0))
        for label, env, C, r, k in tc.pyr_partitions(c):
            _env(monkeypatch, env)
            ctx = _Ctx("pyr", exact)
            ref, cur = ctx.pyrs(name)
            assert cur.return3DEdges(lvl).shape[0] == 0
            for R0, T0 in tc.poses_of(c):
                Ro, To, _, _, ev, _ = ot.track_level(o_ref, o_cur, R0, T0, lvl)
                info = ctx.api.ResidualInfo()
                err, R, T = ctx.opt.trackFrames(ref, cur, R0, T0, lvl, info)
                at = (label, name, lvl)
                assert np.isnan(err) and (info.good_pts_edges, info.bad_pts_edges) == (0, 0), at
                assert np.asarray(T, np.float32).tobytes() == np.asarray(T0, np.float32).tobytes() == np.asarray(To, np.float32).tobytes(), at
                assert np.asarray(R, np.float32).tobytes() == np.asarray(Ro, np.float32).tobytes(), (at, R - Ro)
                if R0 is tc.IDENTITY[0]:
                    assert np.asarray(R, np.float32).tobytes() == np.eye(3, dtype=np.float32).tobytes(), at
                ctx.key(ref, cur, R0, T0)
                assert ctx.trk.last_evals[lvl] == ev, (at, ctx.trk.last_evals.tolist(), ev)
                n += 1
            del ctx
    assert n == 2 * 4 * len(ROW8) and len(ROW8) == 2
