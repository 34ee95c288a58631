"""The matrix of non-default optimizer settings shared by test_optimizer_settings_cpu.py and test_gpu_optimizer_settings.py:
the cases, the two start poses, the seeded pairs and the oracle's runs of them (float sums, double sums, the LM trace).

Every case terminates in the reference: step_size_min > 0 and lambda_fail_fac > 1 everywhere, so a chain of rejected
candidates shrinks its step until the too-small-step exit takes it.  Never add a case whose retry loop has no such exit
(lambda_fail_fac <= 1 with a non-positive step_size_min): the device would leave it only through its MAX_TOTAL_EVALS guard.
Test infrastructure only: nothing under revo_amd/ imports it."""
import functools

import numpy as np

from revo_amd import synth
from revo_amd.settings import ImgPyramidSettings, OptimizerSettings, TrackerSettings, MAX_LEVELS

S160 = ImgPyramidSettings.scaled(160, 120, 3, hist_patch=(5, 0, 0, 0, 0, 0))    # levels 1, 2 below 400 points: the redundant path
S320 = ImgPyramidSettings.scaled(320, 240, 3, hist_patch=(10, 5, 0, 0, 0, 0))
SIZES = {"160": S160, "320": S320}
SEEDS = range(4000, 4016)
NPAIRS = len(SEEDS)

_DAMPED = dict(lambda_initial=(5.0, 1.0, 0.25), lambda_success_fac=0.1, lambda_fail_fac=3.0)
_DAMPED2 = dict(lambda_initial=0.35, lambda_success_fac=0.6, lambda_fail_fac=1.7)
BOTH = ("id", "prior")
PRIOR_TWIST = (0.03, -0.02, 0.02, 0.01, 0.03, -0.01)

# name -> (OptimizerSettings fields: a scalar for every level or a tuple by level, finest first; the starts)
CASES = {
    "gn1": (dict(max_its_per_lvl=1, step_size_min=1e30), BOTH),
    "cap3_nostep": (dict(max_its_per_lvl=3, step_size_min=1e30), BOTH),
    # from the full prior one pair rejects its level-0 candidate with a squared step above 1e-4 and retries (evals[0] = 3 in the
    # oracle, float and double sums): minus half the prior, where every level-0 reject is the too-small-step exit
    "caps123+smin": (dict(max_its_per_lvl=(1, 2, 3), step_size_min=1e-4), ("id", "-prior/2")),
    "eps0": (dict(convergence_eps=0.0), BOTH),
    # from the full prior two of the 16 pairs end a level in a seven-candidate retry chain at the default step_size_min,
    # which the oracle's float and double sums leave at different lengths (14 of 16 equal): half the prior instead
    "eps0.9": (dict(convergence_eps=0.9), ("id", "prior/2")),
    "smin1e-6": (dict(step_size_min=1e-6), BOTH),
    "smin1e-4": (dict(step_size_min=1e-4), BOTH),
    "huber.05+smin": (dict(huber_edge=0.05, step_size_min=1e-4), BOTH),
    "huber3+eps.9": (dict(huber_edge=3.0, convergence_eps=0.9), BOTH),
    # from the prior the tight filter is discontinuous: the reference disagrees with itself by 1.8e-3 at equal counts
    "edist322+smin": (dict(edge_distance_lvl=(3.0, 2.0, 2.0), step_size_min=1e-4), ("id",)),
    "edist1e9+smin": (dict(edge_distance_lvl=1e9, step_size_min=1e-4), BOTH),
    "damped+cap3": (dict(max_its_per_lvl=3, **_DAMPED), BOTH),
    "damped+smin": (dict(step_size_min=1e-4, **_DAMPED), BOTH),
    "damped2+smin": (dict(step_size_min=1e-4, **_DAMPED2), BOTH),
    # never converges by ratio and runs into the noise: for the bitwise tests only
    "free": (dict(convergence_eps=2.0, max_its_per_lvl=5), BOTH),
}
CASES_320 = ("gn1", "caps123+smin", "huber.05+smin", "damped+cap3")
NO_RETRIES = ("gn1", "cap3_nostep")  # step_size_min 1e30: the first rejected candidate ends the level


# one weight / filter field away from the defaults: what the per-point terms see (evaluated with use_edge_filter 0 and 1)
WEIGHT_CASES = {
    "huber.05": dict(huber_edge=0.05),
    "huber3": dict(huber_edge=3.0),
    "huber1e9": dict(huber_edge=1e9),
    "edist322": dict(edge_distance_lvl=(3.0, 2.0, 2.0)),
    "edist1e9": dict(edge_distance_lvl=1e9),
}


def optimizer_settings(name, use_edge_filter=1):
    """OptimizerSettings of a case of CASES or WEIGHT_CASES (None: the defaults)."""
    os_ = OptimizerSettings(use_edge_filter=use_edge_filter)
    fields = {} if name is None else CASES[name][0] if name in CASES else WEIGHT_CASES[name]
    for field, v in fields.items():
        cur = getattr(os_, field)
        if isinstance(cur, (int, float)):
            setattr(os_, field, v)
            continue
        vals = tuple(v) if isinstance(v, tuple) else (v,) * MAX_LEVELS
        for i in range(MAX_LEVELS):
            cur[i] = vals[min(i, len(vals) - 1)]
    assert os_.lambda_fail_fac > 1 and all(os_.step_size_min[i] > 0 for i in range(MAX_LEVELS)), name
    return os_


def tracker_settings(start, check_init=None):
    """"id" runs checkInitializationValues (a no-op from identity); a prior must not be reset by it."""
    chk = (1 if start == "id" else 0) if check_init is None else check_init
    return TrackerSettings(check_init_values=chk)


def start_pose(start):
    """"id": identity; "prior", "prior/2", "-prior/2": exp(PRIOR_TWIST times 1, 1/2, -1/2).  -> (R float32 3x3, T float32 3)"""
    if start == "id":
        return np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
    M = synth.se3_exp(np.array(PRIOR_TWIST) * {"prior": 1.0, "prior/2": 0.5, "-prior/2": -0.5}[start])
    return M[:3, :3].astype(np.float32), M[:3, 3].astype(np.float32)


def matrix(size, with_free=True):
    """[(case, start)] of a size, in a fixed order."""
    names = list(CASES) if size == "160" else [n for n in CASES if n in CASES_320 or n == "free"]
    return [(n, st) for n in names if with_free or n != "free" for st in CASES[n][1]]


@functools.lru_cache(maxsize=None)
def pairs(size):
    return synth.make_pairs(SEEDS, SIZES[size])


@functools.lru_cache(maxsize=None)
def oracle_pyramids(size):
    from oracle import ro
    out = []
    for p in pairs(size):
        o_ref, o_cur = ro.Pyramid(SIZES[size], *p["ref"]), ro.Pyramid(SIZES[size], *p["curr"])
        o_ref.makeKeyframe()
        out.append((o_ref, o_cur))
    return out


def pose_distance(Ra, Ta, Rb, Tb):
    """max of the rotation angle (rad) and the translation distance (m)"""
    return max(synth.rot_angle(Ra, Rb), float(np.linalg.norm(np.asarray(Ta, np.float64) - np.asarray(Tb, np.float64))))


@functools.lru_cache(maxsize=None)
def oracle_runs(size, case, start, double, check_init=None):
    """The oracle's trackFrames of the 16 pairs: per pair a dict of R, T, err, good, bad, status, flags, evals (3 levels) and
    trace (per level the accept = 1 / reject = 0 sequence of the evaluations after the level's first).  Do not modify."""
    from oracle import ro
    s = SIZES[size]
    L = ro.lib()
    ot = ro.Tracker(s, optimizer_settings(case), tracker_settings(start, check_init))
    R0, T0 = start_pose(start)
    buf = np.zeros(16384, np.uint8)
    out = []
    L.ro_set_accum_double(1 if double else 0)
    try:
        for o_ref, o_cur in oracle_pyramids(size):
            L.ro_lm_trace(1)
            r = ot.trackFrames(o_ref, o_cur, R0, T0)
            n = L.ro_lm_trace_get(buf.ctypes.data_as(ro.u8p), len(buf))
            assert n < len(buf)
            tr = buf[:n]
            out.append(dict(R=r["R"], T=r["T"], err=r["err"], good=r["info"].good_pts_edges, bad=r["info"].bad_pts_edges,
                            status=r["status"], flags=r["flags"], evals=tuple(int(x) for x in r["evals"][:s.nLevels()]),
                            trace=tuple(tuple(int(x) & 1 for x in tr[(tr >> 1) == lvl]) for lvl in range(s.nLevels()))))
    finally:
        L.ro_lm_trace(0)
        L.ro_set_accum_double(0)
    for r in out:
        assert all(len(t) == e - 1 for t, e in zip(r["trace"], r["evals"])), (case, start)
    return out


def self_distance(size, case, start):
    """(pairs on which the oracle's float sums and double sums give the same evals, the largest pose distance between the
    two on those pairs): how far the reference is from itself under this case."""
    f, d = oracle_runs(size, case, start, False), oracle_runs(size, case, start, True)
    same = [i for i in range(NPAIRS) if f[i]["evals"] == d[i]["evals"]]
    return same, max([pose_distance(f[i]["R"], f[i]["T"], d[i]["R"], d[i]["T"]) for i in same] or [0.0])


def level_exit(trace, max_its):
    """How the reference left a level, from its accept / reject sequence: 'cap' (max_its iterations were accepted), 'small'
    (a rejected candidate's step was too small: the level ends on a reject), 'conv' (an accepted candidate ended it early:
    the convergence ratio), 'none' (max_its 0)."""
    if not trace:
        return "none"
    if trace[-1] == 0:
        return "small"
    return "cap" if sum(trace) >= max_its else "conv"


FORCED = ("gn1", "cap3_nostep", "caps123+smin")


def check_forced_lengths(case, evals):
    """The evaluation counts the settings of a FORCED case leave no choice about (evals: by level, finest first)."""
    if case == "gn1":  # the first evaluation and one candidate, accepted (the cap) or rejected (the step is below 1e30)
        assert all(e == 2 for e in evals[:3]), (case, evals)
    elif case == "cap3_nostep":  # at most three accepted candidates; the first rejected one ends the level
        assert all(2 <= e <= 4 for e in evals[:3]), (case, evals)
    elif case == "caps123+smin":  # one iteration at level 0; from the case's starts a rejected candidate's squared step is below 1e-4 there
        assert evals[0] == 2, (case, evals)
    else:
        raise KeyError(case)
