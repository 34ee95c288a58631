"""The poses far from the truth shared by test_far_poses_cpu.py and test_gpu_far_poses.py: the scenes, the named poses
(R, T curr -> keyframe, float32), the oracle's pyramids of them and the priors of the whole-tracker tests.

Scene A: 160x120, 3 levels, synth.make_pair(31).  The poses turn the cloud behind the camera (no Z > 0 test exists in the
reference: such points count as good), out of the image altogether (good = 0 with a list that is not empty) or far down the
optical axis (every point on the principal point, Jacobian terms over many decades).

Scene B, the rim scene: 160x120, fx = fy = 128, cx = 80, cy = 60, a depth plane at 2.0 and two different 8x8-block random
binary images.  Every 3-D edge has Z = 2 exactly and the level cameras are 128 / 64 / 32 with integral centres, so every
projection at the identity is an integer pixel and a pure shift T = (kx 2 / fx_l, ky 2 / fy_l, 0) moves every projection of
level l by exactly (kx, ky) pixels: points sit exactly on the rims of `u > 1 && v > 1 && u < w-2 && v < h-2` and of the cost
function's `0 <= u < w`.
Test infrastructure only: nothing under revo_amd/ imports it."""
import functools

import numpy as np

from revo_amd import synth
from revo_amd.settings import ImgPyramidSettings, PLANE_EDGES3D

SA = ImgPyramidSettings.scaled(160, 120, 3, hist_patch=(5, 0, 0, 0, 0, 0))
SB = ImgPyramidSettings(width=160, height=120, fx=128.0, fy=128.0, cx=80.0, cy=60.0, pyr_min_lvl=2,
                        hist_patch=(5, 0, 0, 0, 0, 0))
NLEVELS = 3
SEED_A = 31
PLANE_Z = 2.0
SHIFTS = ((0, 0), (3, 0), (-3, 0), (0, 2), (0, -2), (0.5, 0.25), (7, -5))  # (kx, ky) pixels of the level evaluated


def _rot(axis, deg):
    """Rotation by deg about x (pitch), y (yaw) or z (roll); the entries of a multiple of 90 degrees are exactly 0 / +-1."""
    a = np.deg2rad(float(deg))
    c, s = np.cos(a), np.sin(a)
    if deg % 90 == 0:
        c, s = np.round(c), np.round(s)
    i, j = {"x": (1, 2), "y": (2, 0), "z": (0, 1)}[axis]
    R = np.eye(3)
    R[i, i] = R[j, j] = c
    R[i, j], R[j, i] = -s, s
    return R.astype(np.float32)


def _pose(R=None, T=(0, 0, 0)):
    return (np.eye(3, dtype=np.float32) if R is None else np.asarray(R, np.float32)), np.asarray(T, np.float32)


@functools.lru_cache(maxsize=None)
def pair_a():
    return synth.make_pair(SEED_A, SA)


@functools.lru_cache(maxsize=None)
def pair_b():
    """The rim scene's frames: ref and curr are different block images over the same depth plane."""
    rng = np.random.default_rng(20240)
    out = {}
    for name in ("ref", "curr"):
        blocks = rng.integers(0, 2, (SB.height // 8, SB.width // 8))
        gray = np.where(np.kron(blocks, np.ones((8, 8), np.int64)) > 0, 220, 20).astype(np.uint8)
        out[name] = (np.ascontiguousarray(np.repeat(gray[:, :, None], 3, 2)), np.full((SB.height, SB.width), PLANE_Z, np.float32))
    return out


def pair(scene):
    return pair_a() if scene == "A" else pair_b()


def settings(scene):
    return SA if scene == "A" else SB


@functools.lru_cache(maxsize=None)
def oracle_pyramids(scene):
    """(o_ref made keyframe, o_cur) of a scene.  Do not modify."""
    from oracle import ro
    s, p = settings(scene), pair(scene)
    o_ref, o_cur = ro.Pyramid(s, *p["ref"]), ro.Pyramid(s, *p["curr"])
    o_ref.makeKeyframe()
    return o_ref, o_cur


@functools.lru_cache(maxsize=None)
def depth_stats_a():
    """(median Z, max Z) of scene A's level-0 edge list of the current frame, as float32."""
    z = oracle_pyramids("A")[1].read(PLANE_EDGES3D, 0)[:, 2]
    return np.float32(np.median(z)), np.float32(z.max())


@functools.lru_cache(maxsize=None)
def poses_a():
    """{name: (R, T)} of scene A, in a fixed order."""
    zmed, zmax = depth_stats_a()
    return {
        "identity": _pose(),
        "tx0.5": _pose(T=(0.5, 0, 0)),
        "tx1000": _pose(T=(1000, 0, 0)),
        "yaw20": _pose(_rot("y", 20)),
        "yaw45": _pose(_rot("y", 45)),
        "yaw90": _pose(_rot("y", 90)),
        "yaw180": _pose(_rot("y", 180)),
        "pitch180": _pose(_rot("x", 180)),
        "roll90": _pose(_rot("z", 90)),
        "roll180": _pose(_rot("z", 180)),
        "through": _pose(T=(0, 0, -zmed)),
        "behind": _pose(T=(0, 0, np.float32(-2) * zmax)),
        "tz50": _pose(T=(0, 0, 50)),
        "tz1e4": _pose(T=(0, 0, 1e4)),
        "yaw180+tz": _pose(_rot("y", 180), T=(0, 0, np.float32(2) * zmed)),
    }


def level_camera(scene, lvl):
    """(fx, fy, cx, cy, w, h) of a level, as the reference's CameraPyr scales them (camerapyr.h:139-144)."""
    s = settings(scene)
    k = np.float32(1.0) / np.float32(2 ** lvl)
    return (np.float32(s.fx) * k, np.float32(s.fy) * k, np.float32(s.cx) * k, np.float32(s.cy) * k,
            int(np.float32(s.width) * k), int(np.float32(s.height) * k))


def shift_pose(lvl, kx, ky):
    """Scene B: the pure shift that moves every projection of level lvl by exactly (kx, ky) pixels."""
    fx, fy = level_camera("B", lvl)[:2]
    return _pose(T=(np.float32(kx * PLANE_Z) / fx, np.float32(ky * PLANE_Z) / fy, 0))


def projections(pts, cam, R, T, cost=False):
    """(u, v, Z) of a level's points in float32, operation by operation: X/Z*fx + cx as calcErrorAndBuffers forms it
    (optimizer.cpp:96-97), or with cost=True (fx*X)/Z + cx as evalCostFunction does (tracker.cpp:375-376)."""
    fx, fy, cx, cy = (np.float32(c) for c in cam[:4])
    R, T, p = np.asarray(R, np.float32).reshape(3, 3), np.asarray(T, np.float32).reshape(3), np.asarray(pts, np.float32)
    X, Y, Z = [((R[r, 0] * p[:, 0] + R[r, 1] * p[:, 1]) + R[r, 2] * p[:, 2]) + T[r] for r in range(3)]
    with np.errstate(all="ignore"):
        if cost:
            return (fx * X) / Z + cx, (fy * Y) / Z + cy, Z
        return X / Z * fx + cx, Y / Z * fy + cy, Z


def ulps(a, b):
    """Distance in float32 units in the last place (same-sign ordering of the bit patterns)."""
    def key(x):
        i = np.asarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


def cases(scene):
    """[(name, lvl, R, T)]: every pose of scene A at every level; every shift of scene B at the level it is exact for."""
    out = []
    for lvl in range(NLEVELS):
        if scene == "A":
            out += [(name, lvl, R, T) for name, (R, T) in poses_a().items()]
        else:
            out += [("shift(%g,%g)" % k, lvl) + shift_pose(lvl, *k) for k in SHIFTS]
    return out


def all_cases():
    return [(sc,) + c for sc in ("A", "B") for c in cases(sc)]


# The priors of the whole-tracker tests (scene A).  EMPTY leave no valid point at any level; BEATEN lose the initialisation
# check to the identity by a wide margin (test_far_poses_cpu.py holds both to that); WANDER are tracked with the check off.
EMPTY = ("yaw90", "tx1000")
BEATEN = ("tx0.5", "yaw20", "yaw45", "yaw180", "pitch180", "roll90", "roll180", "through", "behind", "tz50", "tz1e4", "yaw180+tz")
WANDER = ("yaw180", "yaw45", "through")
PRIORS = ("identity",) + EMPTY + BEATEN


def _plain(r):
    err, info, A, b = r
    return dict(err=np.float32(err), good=info.good_pts_edges, bad=info.bad_pts_edges, sum_w=np.float32(info.sum_error_weighted),
                sum_u=np.float32(info.sum_error_unweighted), A=np.array(A, np.float32), b=np.array(b, np.float32))


@functools.lru_cache(maxsize=None)
def oracle_evals(scene):
    """{(name, lvl): (the oracle's evaluation with double sums, with float sums)} under the default OptimizerSettings, each a
    dict of err, good, bad, sum_w, sum_u, A, b.  Do not modify."""
    from oracle import ro
    from revo_amd.settings import OptimizerSettings, TrackerSettings
    o_ref, o_cur = oracle_pyramids(scene)
    ot = ro.Tracker(settings(scene), OptimizerSettings(), TrackerSettings())
    L = ro.lib()
    out = {}
    for name, lvl, R, T in cases(scene):
        L.ro_set_accum_double(1)
        try:
            d = _plain(ot.eval(o_ref, o_cur, R, T, lvl))
        finally:
            L.ro_set_accum_double(0)
        out[(name, lvl)] = (d, _plain(ot.eval(o_ref, o_cur, R, T, lvl)))
    return out


def scaled_distance(got, ref):
    """(error, A, b) distances of an evaluation from `ref` in test_residual_and_normal_equations_parity's scaled norm: relative on
    the error, A over sqrt(diag diag^T), b over sqrt(diag) max(1, sqrt(err)), all of ref.  An entry whose scale is 0 counts 0
    when it is equal and inf when not."""
    with np.errstate(all="ignore"):
        dg = np.diag(ref["A"]).astype(np.float64)

        def rel(d, scale):
            d, scale = np.abs(np.asarray(d, np.float64)), np.asarray(scale, np.float64)
            return float(np.max(np.where(d == 0, 0.0, np.where(scale > 0, d / scale, np.inf))))
        e = float(ref["err"])
        return (rel(float(got["err"]) - e, abs(e)), rel(got["A"].astype(np.float64) - ref["A"], np.sqrt(np.outer(dg, dg))),
                rel(got["b"].astype(np.float64) - ref["b"], np.sqrt(dg) * max(1.0, np.sqrt(e))))


def d_self(scene, name, lvl):
    """The oracle's own float-against-double distance at a case, in scaled_distance's norm; None where the case has no good point."""
    d, f = oracle_evals(scene)[(name, lvl)]
    return None if d["good"] == 0 else scaled_distance(f, d)


@functools.lru_cache(maxsize=None)
def oracle_track(name, check_init, double=False):
    """The oracle's trackFrames of scene A from the prior `name`.  Do not modify."""
    from oracle import ro
    from revo_amd.settings import OptimizerSettings, TrackerSettings
    o_ref, o_cur = oracle_pyramids("A")
    ot = ro.Tracker(SA, OptimizerSettings(), TrackerSettings(check_init_values=check_init))
    R, T = poses_a()[name]
    ro.lib().ro_set_accum_double(1 if double else 0)
    try:
        r = ot.trackFrames(o_ref, o_cur, R, T)
    finally:
        ro.lib().ro_set_accum_double(0)
    return dict(R=r["R"], T=r["T"], err=r["err"], good=r["info"].good_pts_edges, bad=r["info"].bad_pts_edges, status=r["status"],
                flags=r["flags"], evals=tuple(int(x) for x in r["evals"][:NLEVELS]))


# Rim-scene priors (shifts of the coarsest level) at which checkInitializationValues decides differently as soon as ONE rim of
# the cost function's `0 <= u < w && 0 <= v < h` (or its floor) is moved: rule -> (kx, ky).  test_far_poses_cpu.py holds them to that.
RIM_RULES = {"u>0": (-6.75, 0.0), "v>0": (-7.0, 0.25), "u<w-1": (-8.0, -1.0), "v<h-1": (-7.0, 1.0), "trunc>-1": (-7.75, -2.75)}


def rim_cost(lvl, R, T, rule="true"):
    """evalCostFunction on the rim scene in float64 (exact for these terms) under the reference's rule ("true") or with one rim
    moved: "u>0" / "v>0" for `>= 0`, "u<w-1" / "v<h-1" for `< w` / `< h`, "trunc>-1" for a cast in place of floorf behind `> -1`."""
    from revo_amd.settings import OptimizerSettings, PLANE_DT
    o_ref, o_cur = oracle_pyramids("B")
    cam = level_camera("B", lvl)
    w, h = np.float32(cam[4]), np.float32(cam[5])
    u, v, _ = projections(o_cur.read(PLANE_EDGES3D, lvl), cam, R, T, cost=True)
    if rule == "trunc>-1":
        m = (u > -1) & (u < w) & (v > -1) & (v < h)
        iu, iv = u[m].astype(np.int64), v[m].astype(np.int64)
    else:
        m = ((u > 0) if rule == "u>0" else (u >= 0)) & ((v > 0) if rule == "v>0" else (v >= 0)) & \
            (u < (w - 1 if rule == "u<w-1" else w)) & (v < (h - 1 if rule == "v<h-1" else h))
        iu, iv = np.floor(u[m]).astype(np.int64), np.floor(v[m]).astype(np.int64)
    r = o_ref.read(PLANE_DT, lvl)[iv, iu]
    return float(r[~(r > np.float32(OptimizerSettings().edge_distance_lvl[lvl]))].astype(np.float64).sum())
