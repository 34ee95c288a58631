"""The cases shared by the view-gain tests (test_map_gain_cpu.py, test_gpu_map_gain.py).  Small on purpose: the
specification is a Python loop per pose and cell.  They stand on map_seen_cases: its 1/8 m cells, its 16 x 12 camera, its boxes
and its wall scene (a wall in the plane x = 12 of a 24 x 16 x 16 box that leaves the cells y >= 12 open).
Test infrastructure only."""
import functools

import numpy as np

import map_gain_ref as gr
import map_seen_cases as sc
import map_seen_ref as sr

F = np.float32
V = sc.V
KC, SIZE = sc.KC, (16, 12)                  # the 16 x 12 camera: half angles of about 41 and 33 degrees
VIEW = (KC, SIZE)
VIEW8 = (sc.K8, (8, 8))
NARROW = ((24.0, 24.0, 7.5, 5.5, sc.ZMIN, sc.ZMAX), SIZE)    # about 17 x 13 degrees: a frustum thinner than the box
FAR_ONLY = ((8.5, 8.5, 7.5, 5.5, F(4.5), sc.ZMAX), SIZE)     # nothing nearer than 4.5 m counts


def look(pos, axis, sign=1):
    """The pose at `pos` (metres) looking along the world axis `axis` (0, 1, 2) in the direction `sign`: a right-handed frame
    from exact 0 / +-1 entries."""
    z = np.zeros(3)
    z[axis] = sign
    y = np.zeros(3)
    y[(axis + 2) % 3] = -1.0
    T = np.eye(4)
    T[:3, 0], T[:3, 1], T[:3, 2], T[:3, 3] = np.cross(y, z), y, z, pos
    return T.astype(F)


def nudged(T, seed, scale=0.04):
    """T with a small random twist applied: nothing about the result is exact."""
    from revo_amd import synth
    rng = np.random.default_rng(seed)
    return (np.asarray(T, np.float64) @ synth.se3_exp(rng.uniform(-scale, scale, 6))).astype(F)


def bad_pose(kind):
    T = np.eye(4, dtype=F)
    if kind == "nan":
        T[1, 3] = np.nan
    elif kind == "inf":
        T[0, 0] = np.inf
    else:  # not orthogonal
        T[0, 0] = F(1.001)
    return T


# ------------------------------------------------------------------------------------------------------- the wall scene --
@functools.lru_cache(maxsize=None)
def wall():
    """map_seen_cases.wall_scene() with its real seen volume (the specification's), a far wall in the plane x = 23 behind the
    gap and, for the poses that look away, a few voxels outside the box behind the camera."""
    w = sc.wall_scene()
    seen = sr.observe(V, w["lo"], w["n"], w["views"])[0]
    behind = [(-20, y, z) for y in range(4, 12) for z in range(4, 12)]
    back = [(23, y, z) for y in range(10, 16) for z in range(16)]   # a far wall behind the gap: the rays through it end somewhere
    rec = sc.records_at([tuple(c) for c in sr.fr.key_axes(w["rec"]["key"]).tolist()] + behind + back)
    return dict(lo=w["lo"], n=w["n"], rec=rec, seen=seen, view_T=w["views"][0][1], start=w["start"])


FACING_WALL = look((1.0, 0.5, 1.0), 0)      # 0.56 m in front of the wall, every ray ends on it
FACING_GAP = look((1.0, 1.75, 1.0), 0)      # in front of the open cells y >= 12
WALL_POSES = [FACING_WALL, FACING_GAP]


def wall_case(poses, seen=None, view=VIEW, **params):
    w = wall()
    return dict(lo=w["lo"], n=w["n"], rec=w["rec"], seen=w["seen"] if seen is None else seen, view=view, poses=np.stack(poses), params=params)


# ------------------------------------------------------------------------------------------------------ the small boxes --
def plane_records():
    """Voxels in the plane of cells z = 10 behind map_seen_cases' boxes, with holes: some rays hit, some miss."""
    return sc.records_at([(i, j, 10) for i in range(-6, 7) for j in range(-5, 6) if (i + 2 * j) % 5 != 0] + [(0, 0, 8), (2, -1, 7)])


def box_case(lo, n, poses, seen=None, view=VIEW, rec=None, **params):
    rng = np.random.default_rng(sum(n) + 7 * len(poses))
    if seen is None:  # every kind of byte, mostly unseen
        seen = rng.choice(np.array([0, 0, 0, 0, 1, 2, 0x7F, 0x80, 0x81], np.uint8), tuple(n))
    return dict(lo=lo, n=n, rec=plane_records() if rec is None else rec, seen=seen, view=view, poses=np.stack(poses), params=params)


BOX_POSES = [sc.I4, nudged(sc.I4, 1), look((0.9, 0.0, 0.9), 0, -1)]
EMPTY = np.zeros(0, sc.mrr.DTYPE)


def many_poses(k, seed=5):
    """k poses around the identity: the first few exact, the rest nudged."""
    return [sc.I4, look((0.0, 0.0, 2.0), 2, -1)] [:k] + [nudged(sc.I4, seed + i, 0.08) for i in range(max(0, k - 2))]


def cases():
    """name -> dict(lo, n, rec, seen, view, poses, params): every hand-made case of the CPU and the GPU tests."""
    c = {}
    w = wall()
    zero, full = np.zeros(w["n"], np.uint8), np.full(w["n"], 0x7F, np.uint8)
    c["wall, real volume"] = wall_case(WALL_POSES, margin=V)
    c["wall, miss depth"] = wall_case(WALL_POSES, miss_depth=2.0)
    c["wall, nothing seen"] = wall_case([FACING_GAP, look((1.5, 1.0, 1.0), 1)], seen=zero)   # cameras inside the box
    c["wall, all seen"] = wall_case(WALL_POSES + [w["view_T"]], seen=full, miss_depth=1.5)
    c["wall, from outside"] = wall_case([w["view_T"]], miss_depth=3.0)
    c["wall, looking away"] = wall_case([look((-1.0, 1.0, 1.0), 0, -1)], seen=zero, miss_depth=2.0)
    centre = (1.5, 1.0, 1.0)
    c["wall, through each face"] = wall_case([look(centre, a, s) for a in range(3) for s in (1, -1)], seen=zero, view=NARROW, miss_depth=4.0)
    c["wall, nearer than zmin"] = wall_case([look((-1.0, 1.0, 1.0), 0)], seen=zero, view=FAR_ONLY, miss_depth=5.0)
    for lo, n in sc.BOXES:
        tag = "x".join(str(x) for x in n)
        c["box %s" % tag] = box_case(lo, n, BOX_POSES, miss_depth=1.5, margin=sc.M)
    for nz in (1, 3, 4, 5, 33):
        c["tail 3x3x%d" % nz] = box_case((-1, -1, 6), (3, 3, nz), BOX_POSES[:2], miss_depth=1.0 + nz / 16.0)
    for r in range(4):
        c["radius %d" % r] = box_case(sc.LO, sc.N, BOX_POSES[:2], radius=r, miss_depth=1.25, margin_rel=0.03125, margin=0.0)
    twice = np.random.default_rng(2).choice(np.array([0, 1, 1, 2, 0x80], np.uint8), sc.N)
    c["min_views 2"] = box_case(sc.LO, sc.N, BOX_POSES[:2], seen=twice, min_views=2, miss_depth=1.5)
    c["min_views 0"] = box_case(sc.LO, sc.N, BOX_POSES[:1], seen=twice, min_views=0, miss_depth=1.5)
    c["min_count 2"] = box_case(sc.LO, sc.N, BOX_POSES[:2], rec=sc.records_at([(0, 0, 8), (1, 1, 9), (-2, 0, 10)], [1, 2, 3]), min_count=2)
    c["empty map"] = box_case(sc.LO, sc.N, BOX_POSES[:2], rec=EMPTY, miss_depth=1.5)
    c["empty map, holes"] = box_case(sc.LO, sc.N, BOX_POSES[:1], rec=EMPTY)
    c["few steps"] = box_case(sc.LO, sc.N, BOX_POSES[:2], max_steps=3, miss_depth=1.5)
    c["1 pose"] = box_case((-1, -2, 5), (3, 5, 7), many_poses(1), view=VIEW8, miss_depth=1.5)
    c["64 poses"] = box_case((-1, -2, 5), (3, 5, 7), many_poses(64), view=VIEW8, miss_depth=1.5)
    c["65 poses"] = box_case((-1, -2, 5), (3, 5, 7), many_poses(65), view=VIEW8, miss_depth=1.5)
    return c


def device_case():
    """The 65 poses with one NaN, one infinite and one skewed pose among them: what a call with poses in device memory must
    answer with all-zero records."""
    c = dict(cases()["65 poses"])
    poses = c["poses"].copy()
    poses[3], poses[64], poses[40] = bad_pose("nan"), bad_pose("inf"), bad_pose("skew")
    c["poses"] = poses
    return c


@functools.lru_cache(maxsize=None)
def spec(name):
    """The per-cell specification of a case, computed once: (records, info, classes)."""
    c = device_case() if name == "device poses" else cases()[name]
    return gr.view_gain(c["rec"], V, c["lo"], c["n"], c["seen"], c["view"], c["poses"], device_poses=name == "device poses", **c["params"])


def as_array(records):
    """The specification's records as [poses, 4] uint32 in the record's field order."""
    return np.array([[r[f] for f in gr.FIELDS] for r in records], np.uint32).reshape(-1, 4)
